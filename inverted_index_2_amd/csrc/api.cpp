// api.cpp — the C ABI of libii2_hip.so (include/ii2.h): contexts, workspace, segments and their encoders,
// tombstones, the per-device order of look-back kernels, self-test, counters and options.  AND / OR live in
// setop.cpp, the merge in ops.cpp.  There is deliberately no CPU implementation behind any entry point.
#include <algorithm>
#include <functional>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>

#include "internal.h"

using namespace ii2;

static thread_local std::string g_create_err;

// Workspace: reserve the total up front, then carve.
int ii2_ws_reserve(ii2_ctx *ctx, size_t bytes) {
    ctx->ws_used = 0;
    if (bytes <= ctx->ws_cap) return II2_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->ws) (void)hipFree(ctx->ws);
    ctx->ws = nullptr;
    ctx->ws_cap = 0;
    size_t want = align_up(bytes + bytes / 4, 1 << 20);
    if (ii2::dm_malloc_retry((void **)&ctx->ws, want) != hipSuccess) return fail(ctx, II2_ENOMEM, "workspace allocation failed");
    ctx->ws_cap = want;
    return II2_OK;
}

void *ii2_pool_get(ii2_ctx *ctx, int slot, size_t bytes) {
    if (bytes <= ctx->pool_cap[slot] && ctx->pool[slot]) return ctx->pool[slot];
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->pool[slot]) (void)hipFree(ctx->pool[slot]);
    ctx->pool[slot] = nullptr;
    ctx->pool_cap[slot] = 0;
    const size_t want = align_up(bytes + bytes / 8 + 256, 1 << 16);
    if (ii2::dm_malloc_retry((void **)&ctx->pool[slot], want) != hipSuccess) return nullptr;
    ctx->pool_cap[slot] = want;
    return ctx->pool[slot];
}

int ensure_debug(ii2_ctx *ctx, bool clear) {
    const size_t bytes = (size_t)2048 * 8 * sizeof(unsigned long long);
    if (!ctx->d_debug && ii2::dm_malloc_retry((void **)&ctx->d_debug, bytes) != hipSuccess) return fail(ctx, II2_ENOMEM, "debug buffer allocation failed");
    if (clear) HIP_TRY(ctx, hipMemsetAsync(ctx->d_debug, 0, bytes, ctx->stream));
    return II2_OK;
}

bool ii2_profile_pair(ii2_ctx *ctx, hipEvent_t *e0, hipEvent_t *e1) {
    if (ctx->opt_profile_events <= 0) return false;
    if (ctx->prof_calls++ % (uint64_t)ctx->opt_profile_events != 0) return false;   // a timed event pair costs ~10 us of stream idle time
    std::pair<hipEvent_t, hipEvent_t> pr;
    if (!ctx->prof_pool.empty()) { pr = ctx->prof_pool.back(); ctx->prof_pool.pop_back(); }
    else if (hipEventCreate(&pr.first) != hipSuccess || hipEventCreate(&pr.second) != hipSuccess) return false;
    ctx->prof_events.push_back(pr);
    *e0 = pr.first;
    *e1 = pr.second;
    return true;
}

extern "C" {

int ii2_profile_read(ii2_ctx *ctx, double *total_ms, uint64_t *launches) {
    if (!ctx || !total_ms || !launches) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    double tot = 0;
    uint64_t n = 0;
    for (auto &pr : ctx->prof_events) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) { tot += ms; n++; }
        ctx->prof_pool.push_back(pr);
    }
    ctx->prof_events.clear();
    *total_ms = tot;
    *launches = n;
    return II2_OK;
}

int ii2_profile_region(ii2_ctx *ctx, int begin) {
    if (!ctx) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipEvent_t &e = ctx->region_ev[begin ? 0 : 1];
    if (!e) HIP_TRY(ctx, hipEventCreate(&e));
    HIP_TRY(ctx, hipEventRecord(e, ctx->stream));
    return II2_OK;
}

int ii2_profile_region_ms(ii2_ctx *ctx, double *ms) {
    if (!ctx || !ms || !ctx->region_ev[0] || !ctx->region_ev[1]) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipEventSynchronize(ctx->region_ev[1]));
    float f = 0;
    HIP_TRY(ctx, hipEventElapsedTime(&f, ctx->region_ev[0], ctx->region_ev[1]));
    *ms = f;
    return II2_OK;
}

int ii2_abi_version(void) { return II2_ABI_VERSION; }

int ii2_ctx_create(int device, uint32_t flags, ii2_ctx **out) {
    (void)flags;
    if (!out) return II2_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        g_create_err = "no HIP device visible (libii2_hip has no CPU path)";
        return II2_ENODEVICE;
    }
    if (device < 0 || device >= n) { g_create_err = "device ordinal out of range"; return II2_EINVAL; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { g_create_err = "hipGetDeviceProperties failed"; return II2_EHIP; }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_create_err = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
        return II2_ENODEVICE;
    }
    if (hipSetDevice(device) != hipSuccess) { g_create_err = "hipSetDevice failed"; return II2_EHIP; }
    ii2_ctx *ctx = new (std::nothrow) ii2_ctx();
    if (!ctx) return II2_ENOMEM;
    ctx->device = device;
    ctx->cu_count = prop.multiProcessorCount;
    dm_user(+1);
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipHostMalloc((void **)&ctx->h_mail, II2_MAIL_WORDS * sizeof(uint64_t)) != hipSuccess ||
        ii2::dm_malloc_retry((void **)&ctx->d_mail, II2_MAIL_WORDS * sizeof(uint64_t)) != hipSuccess) {
        g_create_err = "context resource allocation failed";
        ii2_ctx_destroy(ctx);
        return II2_EHIP;
    }
    // the merge tile kernel's event counters: zeroed here, on the context's stream (ahead of every launch), and never again
    if (ii2::dm_malloc_retry((void **)&ctx->d_merge_events, ii2::ME_COUNT * sizeof(unsigned long long)) != hipSuccess ||
        hipMemsetAsync(ctx->d_merge_events, 0, ii2::ME_COUNT * sizeof(unsigned long long), ctx->stream) != hipSuccess) {
        g_create_err = "context resource allocation failed";
        ii2_ctx_destroy(ctx);
        return II2_EHIP;
    }
    *out = ctx;
    return II2_OK;
}

void ii2_ctx_destroy(ii2_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    ii2_lookback_forget(ctx);
    ii2_comm_destroy_internal(ctx);
    if (ctx->ws) (void)hipFree(ctx->ws);
    if (ctx->aux) (void)hipFree(ctx->aux);
    if (ctx->h_small_in) (void)hipHostFree(ctx->h_small_in);
    if (ctx->h_small_out) (void)hipHostFree(ctx->h_small_out);
    if (ctx->d_small_in) (void)hipFree(ctx->d_small_in);
    if (ctx->d_small_out) (void)hipFree(ctx->d_small_out);
    if (ctx->h_segs) (void)hipHostFree(ctx->h_segs);
    if (ctx->d_segs) (void)hipFree(ctx->d_segs);
    for (uint8_t *q : ctx->pool) if (q) (void)hipFree(q);
    if (ctx->d_debug) (void)hipFree(ctx->d_debug);
    if (ctx->d_lb) (void)hipFree(ctx->d_lb);
    if (ctx->d_small) (void)hipFree(ctx->d_small);
    if (ctx->d_um_bits) (void)hipFree(ctx->d_um_bits);
    if (ctx->d_thr) (void)hipFree(ctx->d_thr);
    if (ctx->h_um) (void)hipHostFree(ctx->h_um);
    if (ctx->d_ir) (void)hipFree(ctx->d_ir);
    if (ctx->h_ir) (void)hipHostFree(ctx->h_ir);
    if (ctx->d_an) (void)hipFree(ctx->d_an);
    if (ctx->d_batch) (void)hipFree(ctx->d_batch);
    if (ctx->h_batch) (void)hipHostFree(ctx->h_batch);
    if (ctx->d_merge_events) (void)hipFree(ctx->d_merge_events);
    if (ctx->d_mail) (void)hipFree(ctx->d_mail);
    if (ctx->h_mail) (void)hipHostFree(ctx->h_mail);
    for (hipEvent_t e : ctx->region_ev) if (e) (void)hipEventDestroy(e);
    for (auto *v : {&ctx->prof_events, &ctx->prof_pool})
        for (auto &pr : *v) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    dm_user(-1);                 // the last context gives the cached segment arrays back (devmem.cpp)
    delete ctx;
}

const char *ii2_last_error(const ii2_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int ii2_ctx_sync(ii2_ctx *ctx) {
    if (!ctx) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // asynchronous two-list ANDs since the last look: did a bounded wait of any of them run out?  (its count is all ones, or -
    // when the workgroup gave up after the last one had stored the count - its ids are incomplete)  Those a synchronous call
    // or the records' reset came after were looked at then (lb_note_pending).
    lb_fold_pending(ctx);
    bool failed = ctx->lb_async_failed;
    ctx->lb_async_failed = false;
    if (ctx->lb_pending && ctx->d_lb) {
        unsigned long long e = 0;
        const uint32_t first = ctx->lb_pending;
        ctx->lb_pending = 0;
        HIP_TRY(ctx, hipMemcpy(&e, ctx->d_lb, sizeof e, hipMemcpyDeviceToHost));
        failed |= e >= first && e <= ctx->lb_epoch;
    }
    if (failed)
        return fail(ctx, II2_EHIP, "ii2_intersect_async: a workgroup's bounded wait ran out (that call's count is all ones or its ids are incomplete); repeat it with ii2_intersect");
    return II2_OK;
}

void *ii2_ctx_stream(ii2_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }
int ii2_ctx_device(const ii2_ctx *ctx) { return ctx ? ctx->device : -1; }

int ii2_dev_alloc(ii2_ctx *ctx, size_t bytes, void **dptr) {
    if (!ctx || !dptr) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ii2::dm_malloc_retry(dptr, bytes ? bytes : 16) != hipSuccess) return fail(ctx, II2_ENOMEM, "hipMalloc failed");
    return II2_OK;
}
int ii2_dev_free(ii2_ctx *ctx, void *dptr) {
    if (!ctx) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipFree(dptr));
    return II2_OK;
}
int ii2_copy_h2d(ii2_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (!ctx) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return II2_OK;
}
int ii2_copy_d2h(ii2_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (!ctx) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return II2_OK;
}

}  // extern "C"

// ---- segments -----------------------------------------------------------------------------
static void seg_release(ii2_seg *s) {
    if (!s) return;
    if (s->born) (void)hipStreamSynchronize(s->born);     // never finished (an early exit): kernels of that call may still be writing its arrays
    if (s->in_slab) { delete s; return; }       // the store's slab holds every array (ii2_merge_small)
    // (devmem.cpp: the arrays go back to the size-class cache; no driver call, no device-wide wait)
    dm_free(s->d_blk_off);
    if (!s->store) {          // not yet handed to a store: still owned directly
        dm_free(s->d_skip);
        dm_free(s->d_payload);
    }
    dm_free(s->d_last_doc);
    dm_free(s->d_cnt);
    dm_free(s->d_blk_list);
    delete s;
}

// reads back the driver-choice statistics of single-list segments and the host blk_off mirror
// the three per-list / per-block arrays every segment carries next to its DV1 arrays
static int seg_alloc_meta(ii2_ctx *ctx, ii2_seg *seg) {
    if (dm_alloc((void **)&seg->d_last_doc, (seg->n_lists + 1) * sizeof(uint32_t)) != hipSuccess)
        return fail(ctx, II2_ENOMEM, "segment allocation failed");
    if (dm_alloc((void **)&seg->d_cnt, (seg->n_lists + 1) * sizeof(uint32_t)) != hipSuccess ||
        dm_alloc((void **)&seg->d_blk_list, (seg->n_blocks + 1) * sizeof(uint32_t)) != hipSuccess)
        return fail(ctx, II2_ENOMEM, "segment allocation failed");
    return II2_OK;
}

// have_meta: the encoder filled d_cnt / d_last_doc / d_blk_list from the CSR it encoded (no list has to be decoded for them)
// everything a finished segment still needs, enqueued (no wait): the caller waits for the stream and then calls seg_finish_done
static int seg_finish_enqueue(ii2_ctx *ctx, ii2_seg *seg, bool have_meta, bool *count_view_out) {
    if (!seg->store) {
        seg->store = std::make_shared<ii2_seg_store>();
        seg->store->d_skip = seg->d_skip;
        seg->store->d_payload = seg->d_payload;
    }
    if (!have_meta) {
        if (int rcm = seg_alloc_meta(ctx, seg)) return rcm;
        HIP_TRY(ctx, hipMemsetAsync(seg->d_blk_list, 0xFF, (seg->n_blocks + 1) * sizeof(uint32_t), ctx->stream));
        HIP_TRY(ctx, launch_list_last_doc(seg->d_blk_off, seg->d_skip, seg->d_payload, seg->n_lists, seg->d_cnt, seg->d_blk_list, seg->d_last_doc,
                                          ctx->stream));
    }
    if (seg->n_lists <= ii2_seg::SPAN_MIRROR_MAX) {      // (a segment of many lists mirrors them when a query first asks: ii2_seg_host_blk_off)
        seg->h_blk_off.resize(seg->n_lists + 1);
        HIP_TRY(ctx, hipMemcpyAsync(seg->h_blk_off.data(), seg->d_blk_off, (seg->n_lists + 1) * sizeof(uint32_t),
                                    hipMemcpyDeviceToHost, ctx->stream));
    }
    // the lists' spans (what a query's path choice looks at), mirrored now so that no query has to fetch them
    if (seg->n_lists && seg->n_lists <= ii2_seg::SPAN_MIRROR_MAX) {
        if (int rcw = ii2_ws_reserve(ctx, align_up(3 * seg->n_lists * sizeof(uint32_t)) + 256)) return rcw;
        uint32_t *d_sp = ws_take<uint32_t>(ctx, 3 * seg->n_lists);
        HIP_TRY(ctx, launch_list_spans(seg->d_blk_off, seg->d_skip, seg->d_last_doc, seg->n_lists, d_sp, ctx->stream));
        seg->h_spans.resize(3 * seg->n_lists);
        HIP_TRY(ctx, hipMemcpyAsync(seg->h_spans.data(), d_sp, 3 * seg->n_lists * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    // a view's postings: the sum of its lists' counts (the store's total would make every merge of a few of its lists plan,
    // clear and launch for the whole store: milliseconds of fills and empty workgroups per call)
    const bool count_view = seg->is_view && seg->n_lists && seg->d_cnt;
    if (count_view) {
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_mail + 16, 0, sizeof(uint64_t), ctx->stream));
        HIP_TRY(ctx, launch_sum_u32(seg->d_cnt, seg->n_lists, ctx->d_mail + 16, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_mail + 16, ctx->d_mail + 16, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    *count_view_out = count_view;
    return II2_OK;
}
static void seg_finish_done(ii2_ctx *ctx, ii2_seg *seg, bool count_view) {
    if (count_view) seg->n_postings = std::min<uint64_t>(seg->n_postings, ctx->h_mail[16]);
    seg->born = nullptr;                                    // finished: from here on the caller's contract governs its lifetime
}
static int seg_finish(ii2_ctx *ctx, ii2_seg *seg, bool have_meta = false) {
    bool count_view = false;
    if (int rc = seg_finish_enqueue(ctx, seg, have_meta, &count_view)) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    seg_finish_done(ctx, seg, count_view);
    return II2_OK;
}

// encode from device-resident CSR (d_post_off, d_values) — unlocked
int ii2_seg_encode_dev_unlocked(ii2_ctx *ctx, uint64_t n_lists, const uint64_t *d_post_off, const uint32_t *d_values,
                                uint64_t n_postings, ii2_seg **out) {
    hipStream_t st = ctx->stream;
    std::unique_ptr<ii2_seg, void (*)(ii2_seg *)> seg(new (std::nothrow) ii2_seg(), seg_release);
    if (!seg) return II2_ENOMEM;
    seg->device = ctx->device;
    seg->born = ctx->stream;
    seg->n_lists = n_lists;
    seg->n_postings = n_postings;
    const uint64_t nb_bound = n_postings / II2_DV1_BLOCK + n_lists + 1;
    if (nb_bound >= (1ull << 31)) return fail(ctx, II2_ERANGE, "too many DV1 blocks for one segment");
    if (dm_alloc((void **)&seg->d_blk_off, (n_lists + 1) * sizeof(uint32_t)) != hipSuccess)
        return fail(ctx, II2_ENOMEM, "segment allocation failed");
    // scratch comes out of the context's grow-only workspace (sized by the upper bound of the block count)
    const size_t tmpb = scan_temp_bytes((size_t)std::max<uint64_t>(n_lists + 1, nb_bound + 1));
    if (int rcw = ii2_ws_reserve(ctx, align_up((n_lists + 1) * sizeof(uint32_t)) + align_up(tmpb) + align_up((nb_bound + 1) * sizeof(uint32_t)) +
                                          align_up((nb_bound + 1) * sizeof(uint64_t)) + 4096))
        return rcw;
    uint32_t *d_nblk = ws_take<uint32_t>(ctx, n_lists + 1);
    void *d_scan_tmp = ws_take<uint8_t>(ctx, tmpb);
    uint32_t *d_sizes = ws_take<uint32_t>(ctx, nb_bound + 1);
    uint64_t *d_boff = ws_take<uint64_t>(ctx, nb_bound + 1);
    HIP_TRY(ctx, launch_enc_list_blocks(d_post_off, n_lists, d_nblk, st));
    HIP_TRY(ctx, scan_excl_u32(d_scan_tmp, tmpb, d_nblk, seg->d_blk_off, n_lists + 1, st));
    uint32_t nb32 = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&nb32, seg->d_blk_off + n_lists, sizeof nb32, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const uint64_t nb = nb32;
    seg->n_blocks = nb;
    if (dm_alloc((void **)&seg->d_skip, (nb + 1) * sizeof(ii2_skip)) != hipSuccess)
        return fail(ctx, II2_ENOMEM, "segment allocation failed");
    HIP_TRY(ctx, launch_enc_block_sizes(d_post_off, seg->d_blk_off, n_lists, d_values, nb, d_sizes, seg->d_skip, st));
    HIP_TRY(ctx, scan_excl_u32_to_u64(d_scan_tmp, tmpb, d_sizes, d_boff, nb + 1, st));
    uint64_t nbytes = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&nbytes, d_boff + nb, sizeof nbytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (nbytes >= 0xFFFFFFF0ull) return fail(ctx, II2_ERANGE, "segment payload exceeds the 4 GiB DV1 limit; split the segment");
    seg->n_bytes = nbytes;
    if (dm_alloc((void **)&seg->d_payload, nbytes + 16) != hipSuccess) return fail(ctx, II2_ENOMEM, "segment allocation failed");
    HIP_TRY(ctx, hipMemsetAsync(seg->d_payload + nbytes, 0, 16, st));
    if (int rcm = seg_alloc_meta(ctx, seg.get())) return rcm;
    HIP_TRY(ctx, hipMemsetAsync(seg->d_blk_list + nb, 0xFF, sizeof(uint32_t), st));         // (the entry past the last block, as k_list_last_doc leaves it)
    HIP_TRY(ctx, launch_enc_write(d_post_off, seg->d_blk_off, n_lists, d_values, nb, d_boff, seg->d_skip,
                                  seg->d_payload, n_postings, seg->d_blk_list, st));
    HIP_TRY(ctx, launch_enc_list_meta(d_post_off, d_values, n_lists, seg->d_cnt, seg->d_last_doc, st));
    int rc = seg_finish(ctx, seg.get(), true);
    if (rc) return rc;
    seg->born = nullptr;
    *out = seg.release();
    return II2_OK;
}

// encode from device-resident CSR in ONE pass over the ids (encode_stream.hip) - the tail of Shard.Merge (shard.go:207 ->
// file/writer.go:32-59).  The caller knows the number of non-empty lists and an upper bound of the payload (a merge: the inputs'
// payload bytes + 5 per input block - a merged gap is never longer than the gap its posting had in its input list, and only
// the inputs' block-first ids had none), so every array is allocated before the first kernel and nothing is read back until the
// end.  Falls back to the two-pass encoder above when a bounded wait of the look-back runs out or the bound does not hold.
int ii2_seg_encode_stream_unlocked(ii2_ctx *ctx, uint64_t n_lists, const uint64_t *d_post_off, const uint32_t *d_values, uint64_t n_postings,
                                   uint64_t n_nonempty, uint64_t payload_bound, ii2_seg **out) {
    hipStream_t st = ctx->stream;
    if (!ctx->opt_encode_stream || n_postings == 0) return ii2_seg_encode_dev_unlocked(ctx, n_lists, d_post_off, d_values, n_postings, out);
    std::unique_ptr<ii2_seg, void (*)(ii2_seg *)> seg(new (std::nothrow) ii2_seg(), seg_release);
    if (!seg) return II2_ENOMEM;
    seg->device = ctx->device;
    seg->born = ctx->stream;
    seg->n_lists = n_lists;
    seg->n_postings = n_postings;
    const uint64_t nb_bound = n_postings / II2_DV1_BLOCK + std::min<uint64_t>(n_nonempty, n_lists) + 1;
    if (nb_bound >= (1ull << 31)) return fail(ctx, II2_ERANGE, "too many DV1 blocks for one segment");
    const uint64_t cap = std::min<uint64_t>(std::min<uint64_t>(payload_bound, 5ull * n_postings), 0xFFFFFFEFull);
    seg->n_blocks = nb_bound;                      // (sizes the per-block arrays; the exact count comes back with the result)
    if (dm_alloc((void **)&seg->d_blk_off, (n_lists + 1) * sizeof(uint32_t)) != hipSuccess ||
        dm_alloc((void **)&seg->d_skip, (nb_bound + 1) * sizeof(ii2_skip)) != hipSuccess ||
        dm_alloc((void **)&seg->d_payload, cap + 16) != hipSuccess)
        return fail(ctx, II2_ENOMEM, "segment allocation failed");
    if (int rcm = seg_alloc_meta(ctx, seg.get())) return rcm;
    const size_t tmpb = scan_temp_bytes((size_t)n_lists + 1);
    const size_t n_part = (size_t)((n_postings + 1023) / 1024) + 1;       // one word per 1024 output positions (k_enc_partition)
    if (int rcw = ii2_ws_reserve(ctx, align_up((n_lists + 1) * sizeof(uint32_t)) + align_up(tmpb) + align_up(n_part * sizeof(uint32_t)) + 4096)) return rcw;
    uint32_t *d_nblk = ws_take<uint32_t>(ctx, n_lists + 1);
    void *d_scan_tmp = ws_take<uint8_t>(ctx, tmpb);
    uint32_t *d_part = ws_take<uint32_t>(ctx, n_part);
    HIP_TRY(ctx, launch_enc_list_blocks(d_post_off, n_lists, d_nblk, st));
    HIP_TRY(ctx, scan_excl_u32(d_scan_tmp, tmpb, d_nblk, seg->d_blk_off, n_lists + 1, st));
    if (int rcn = lb_note_pending(ctx)) return rcn;       // (the give-ups of asynchronous launches before this one stay reported)
    LookBack lb;
    if (int rcl = ii2_lookback_prepare(ctx, (size_t)enc_stream_workgroups(n_postings), &lb)) return rcl;
    ctx->lb_pending = 0;                           // (this call looks at its own result below)
    if (ctx->opt_encode_stream < 0) lb.spin = ctx->opt_encode_stream == -2 ? LB_SPIN_LATE : LB_SPIN_EARLY;      // tests: a wait runs out (-2: late), the two-pass encoder takes over
    uint64_t *d_res = ctx->d_mail + 8;
    unsigned long long *d_dbg = nullptr;
    if (ctx->opt_debug_stamps == 3) {              // diagnostics: the encoder's cycle counters
        if (int rcd = ensure_debug(ctx, true)) return rcd;
        d_dbg = ctx->d_debug;
    }
    if (int rcq = ii2_lookback_launch(ctx, true, [&] {
            return launch_enc_stream(d_post_off, d_values, seg->d_blk_off, n_lists, n_postings, seg->d_skip, seg->d_payload, cap, seg->d_blk_list,
                                     d_part, d_res, lb, d_dbg, st);
        })) return rcq;
    HIP_TRY(ctx, launch_enc_list_meta(d_post_off, d_values, n_lists, seg->d_cnt, seg->d_last_doc, st));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_mail + 8, d_res, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_mail + II2_MAIL_LB_OWN, ctx->d_lb, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    // the mirrors a finished segment keeps (list spans of small segments) depend on nothing the host still has to learn: they are
    // enqueued behind the encoder and ONE wait serves the byte count and them
    bool count_view = false;
    if (int rcf = seg_finish_enqueue(ctx, seg.get(), true, &count_view)) return rcf;
    HIP_TRY(ctx, hipStreamSynchronize(st));
    lb_fold_pending(ctx);
    const uint64_t nbytes = ctx->h_mail[8], nb = ctx->h_mail[9];
    // a bounded wait ran out (the byte count is all ones - or looks valid when the workgroup gave up after the last one had
    // stored it: the error word tells), or the bound did not hold: the exact two-pass form
    if (nbytes == ~0ull || ctx->h_mail[II2_MAIL_LB_OWN] == lb.epoch || nb > nb_bound) {
        ctx->lb_fallbacks++;
        seg.reset();
        return ii2_seg_encode_dev_unlocked(ctx, n_lists, d_post_off, d_values, n_postings, out);
    }
    seg->n_blocks = nb;
    seg->n_bytes = nbytes;
    seg_finish_done(ctx, seg.get(), count_view);
    *out = seg.release();
    return II2_OK;
}

// decode into device buffers — unlocked.  d_post_off may be null.
int ii2_seg_decode_dev_unlocked(ii2_ctx *ctx, const ii2_seg *seg, uint64_t *d_post_off, uint32_t *d_values) {
    hipStream_t st = ctx->stream;
    const uint64_t nb = seg->n_blocks;
    const size_t tmpb = scan_temp_bytes((size_t)nb + 1);
    if (int rcw = ii2_ws_reserve(ctx, align_up((nb + 1) * sizeof(uint32_t)) + align_up((nb + 1) * sizeof(uint64_t)) + align_up(tmpb) + 4096)) return rcw;
    uint32_t *d_counts = ws_take<uint32_t>(ctx, nb + 1);
    uint64_t *d_bpo = ws_take<uint64_t>(ctx, nb + 1);
    void *d_scan_tmp = ws_take<uint8_t>(ctx, tmpb);
    HIP_TRY(ctx, launch_dec_block_counts(seg->d_skip, seg->d_payload, nb, d_counts, st));
    HIP_TRY(ctx, scan_excl_u32_to_u64(d_scan_tmp, tmpb, d_counts, d_bpo, nb + 1, st));
    if (d_values) HIP_TRY(ctx, launch_dec_write(seg->d_skip, seg->d_payload, nb, d_bpo, d_values, st));
    if (d_post_off) HIP_TRY(ctx, launch_gather_post_off(seg->d_blk_off, d_bpo, seg->n_lists, d_post_off, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return II2_OK;
}

extern "C" {

int ii2_seg_encode(ii2_ctx *ctx, uint64_t n_lists, const uint64_t *post_off, const uint32_t *values, int where, ii2_seg **out) {
    if (!ctx || !post_off || !out || (where != II2_HOST && where != II2_DEVICE)) return fail(ctx, II2_EINVAL, "ii2_seg_encode: bad argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *out = nullptr;
    if (where == II2_DEVICE) {
        uint64_t n = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&n, post_off + n_lists, sizeof n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return ii2_seg_encode_dev_unlocked(ctx, n_lists, post_off, values, n, out);
    }
    const uint64_t n = post_off[n_lists];
    for (uint64_t l = 0; l < n_lists; l++)
        if (post_off[l + 1] < post_off[l]) return fail(ctx, II2_EINVAL, "ii2_seg_encode: post_off must be non-decreasing");
    if (n && !values) return fail(ctx, II2_EINVAL, "ii2_seg_encode: values is NULL");
    uint64_t *dpo = (uint64_t *)ii2_pool_get(ctx, 0, (n_lists + 1) * sizeof(uint64_t));
    uint32_t *dv = (uint32_t *)ii2_pool_get(ctx, 1, n * sizeof(uint32_t));
    if (!dpo || !dv) return fail(ctx, II2_ENOMEM, "encode staging allocation failed");
    HIP_TRY(ctx, hipMemcpyAsync(dpo, post_off, (n_lists + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    if (n) HIP_TRY(ctx, hipMemcpyAsync(dv, values, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    return ii2_seg_encode_dev_unlocked(ctx, n_lists, dpo, dv, n, out);
}

int ii2_seg_import(ii2_ctx *ctx, uint64_t n_lists, uint64_t n_postings, uint64_t n_blocks, uint64_t n_bytes, const uint32_t *blk_off,
                   const ii2_skip *skip, const uint8_t *payload, int where, ii2_seg **out) {
    if (!ctx || !blk_off || !skip || !out) return fail(ctx, II2_EINVAL, "ii2_seg_import: bad argument");
    if (n_blocks > 0xFFFFFFFEull || n_bytes > 0xFFFFFFFFull) return fail(ctx, II2_EINVAL, "ii2_seg_import: a segment holds < 2^32 blocks and payload bytes");
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *out = nullptr;
    const hipMemcpyKind kind = where == II2_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    std::unique_ptr<ii2_seg, void (*)(ii2_seg *)> seg(new (std::nothrow) ii2_seg(), seg_release);
    if (!seg) return II2_ENOMEM;
    seg->device = ctx->device;
    seg->born = ctx->stream;
    seg->n_lists = n_lists;
    seg->n_postings = n_postings;
    // the closing entries must agree with the stated array lengths: nothing below reads past those lengths
    uint32_t nb = 0;
    ii2_skip last;
    if (where == II2_HOST) {
        nb = blk_off[n_lists];
        last = skip[n_blocks];
    } else {
        HIP_TRY(ctx, hipMemcpyAsync(&nb, blk_off + n_lists, sizeof nb, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&last, skip + n_blocks, sizeof last, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (nb != n_blocks) return fail(ctx, II2_EINVAL, "ii2_seg_import: malformed DV1 segment (blk_off[n_lists] differs from n_blocks)");
    if (last.byte_off != n_bytes) return fail(ctx, II2_EINVAL, "ii2_seg_import: malformed DV1 segment (skip[n_blocks].byte_off differs from n_bytes)");
    seg->n_blocks = nb;
    seg->n_bytes = last.byte_off;
    if (seg->n_bytes && !payload) return fail(ctx, II2_EINVAL, "ii2_seg_import: payload is NULL");
    if (dm_alloc((void **)&seg->d_blk_off, (n_lists + 1) * sizeof(uint32_t)) != hipSuccess ||
        dm_alloc((void **)&seg->d_skip, ((uint64_t)nb + 1) * sizeof(ii2_skip)) != hipSuccess ||
        dm_alloc((void **)&seg->d_payload, seg->n_bytes + 16) != hipSuccess)
        return fail(ctx, II2_ENOMEM, "segment allocation failed");
    HIP_TRY(ctx, hipMemcpyAsync(seg->d_blk_off, blk_off, (n_lists + 1) * sizeof(uint32_t), kind, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(seg->d_skip, skip, ((uint64_t)nb + 1) * sizeof(ii2_skip), kind, ctx->stream));
    if (seg->n_bytes) HIP_TRY(ctx, hipMemcpyAsync(seg->d_payload, payload, seg->n_bytes, kind, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(seg->d_payload + seg->n_bytes, 0, 16, ctx->stream));
    {   // refuse structurally broken input before any kernel walks it
        uint32_t *d_bad = (uint32_t *)ctx->d_mail;
        uint32_t bad = 0;
        HIP_TRY(ctx, hipMemsetAsync(d_bad, 0, sizeof(uint32_t), ctx->stream));
        HIP_TRY(ctx, launch_validate_seg(seg->d_blk_off, n_lists, seg->d_skip, nb, seg->n_bytes, d_bad, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (bad) {
            // the arrays are not yet owned by a store: seg_release frees them
            return fail(ctx, II2_EINVAL, "ii2_seg_import: malformed DV1 segment (offsets not monotone / out of range)");
        }
    }
    int rc = seg_finish(ctx, seg.get());
    if (rc) return rc;
    {   // block fill rule (every block full but a list's last): the merge places decoded blocks by it
        uint32_t *d_bad = (uint32_t *)ctx->d_mail;
        uint32_t bad = 0;
        HIP_TRY(ctx, hipMemsetAsync(d_bad, 0, sizeof(uint32_t), ctx->stream));
        HIP_TRY(ctx, launch_validate_counts(seg->d_blk_off, seg->d_blk_list, seg->d_skip, seg->d_payload, nb, d_bad, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (bad) return fail(ctx, II2_EINVAL, "ii2_seg_import: malformed DV1 segment (a block that is not its list's last must hold 256 postings)");
    }
    {   // the caller's n_postings sizes the decode buffers (ii2_seg_decode): it must be the count the blocks really hold
        uint64_t *d_sum = ctx->d_mail + 8;
        uint64_t sum = 0;
        HIP_TRY(ctx, hipMemsetAsync(d_sum, 0, sizeof(uint64_t), ctx->stream));
        HIP_TRY(ctx, launch_sum_u32(seg->d_cnt, n_lists, d_sum, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&sum, d_sum, sizeof sum, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (sum != n_postings) return fail(ctx, II2_EINVAL, "ii2_seg_import: n_postings differs from the number of postings the blocks hold");
    }
    seg->born = nullptr;
    *out = seg.release();
    return II2_OK;
}

int ii2_seg_decode(ii2_ctx *ctx, const ii2_seg *seg, uint64_t *post_off, uint32_t *values, int where) {
    if (!ctx || !seg) return fail(ctx, II2_EINVAL, "ii2_seg_decode: bad argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (where == II2_DEVICE) return ii2_seg_decode_dev_unlocked(ctx, seg, post_off, values);
    uint64_t *dpo = (uint64_t *)ii2_pool_get(ctx, 0, (seg->n_lists + 1) * sizeof(uint64_t));
    uint32_t *dv = (uint32_t *)ii2_pool_get(ctx, 1, seg->n_postings * sizeof(uint32_t));
    if (!dpo || !dv) return fail(ctx, II2_ENOMEM, "decode staging allocation failed");
    int rc = ii2_seg_decode_dev_unlocked(ctx, seg, dpo, values ? dv : nullptr);
    if (rc) return rc;
    if (post_off) HIP_TRY(ctx, hipMemcpyAsync(post_off, dpo, (seg->n_lists + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (values && seg->n_postings)
        HIP_TRY(ctx, hipMemcpyAsync(values, dv, seg->n_postings * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return II2_OK;
}

int ii2_seg_export(ii2_ctx *ctx, const ii2_seg *seg, uint32_t *blk_off, ii2_skip *skip, uint8_t *payload) {
    if (!ctx || !seg) return fail(ctx, II2_EINVAL, "ii2_seg_export: bad argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    if (blk_off) HIP_TRY(ctx, hipMemcpyAsync(blk_off, seg->d_blk_off, (seg->n_lists + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (skip) HIP_TRY(ctx, hipMemcpyAsync(skip, seg->d_skip, (seg->n_blocks + 1) * sizeof(ii2_skip), hipMemcpyDeviceToHost, ctx->stream));
    if (payload && seg->n_bytes) HIP_TRY(ctx, hipMemcpyAsync(payload, seg->d_payload, seg->n_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return II2_OK;
}

int ii2_seg_get_info(const ii2_seg *seg, ii2_seg_info *info) {
    if (!seg || !info) return II2_EINVAL;
    info->n_lists = seg->n_lists;
    info->n_postings = seg->n_postings;
    info->n_blocks = seg->n_blocks;
    info->n_bytes = seg->n_bytes;
    return II2_OK;
}

// the derived arrays as the kernels and the path choice read them: copies only (one wait, no kernel)
int ii2_seg_export_meta(ii2_ctx *ctx, const ii2_seg *seg, uint32_t *cnt, uint32_t *last_doc, uint32_t *blk_list, uint32_t *spans,
                        ii2_seg_meta_info *info) {
    if (!ctx || !seg || seg->device != ctx->device) return fail(ctx, II2_EINVAL, "ii2_seg_export_meta: bad argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nl = (size_t)seg->n_lists * sizeof(uint32_t);
    if (cnt && nl) HIP_TRY(ctx, hipMemcpyAsync(cnt, seg->d_cnt, nl, hipMemcpyDeviceToHost, ctx->stream));
    if (last_doc && nl) HIP_TRY(ctx, hipMemcpyAsync(last_doc, seg->d_last_doc, nl, hipMemcpyDeviceToHost, ctx->stream));
    if (blk_list) HIP_TRY(ctx, hipMemcpyAsync(blk_list, seg->d_blk_list, (seg->n_blocks + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const bool mirrored = seg->h_spans.size() == 3 * seg->n_lists;       // (what setop.cpp asks before it reads the mirror)
    if (spans && mirrored && nl) std::memcpy(spans, seg->h_spans.data(), 3 * nl);
    if (info) {
        info->n_postings = seg->n_postings;
        info->merge_blocks = seg->merge_blocks();
        info->merge_bytes = seg->merge_bytes();
        info->is_view = seg->is_view ? 1u : 0u;
        info->spans_mirrored = mirrored ? 1u : 0u;
    }
    return II2_OK;
}

// what a query has cached for a list: nothing is built here (one wait when the words are copied, no kernel)
int ii2_seg_dense_form(ii2_ctx *ctx, const ii2_seg *seg, uint64_t list_idx, uint64_t info[4], uint32_t *words, uint64_t cap) {
    if (!ctx || !seg || !info || seg->device != ctx->device || list_idx >= seg->n_lists) return fail(ctx, II2_EINVAL, "ii2_seg_dense_form: bad argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc0 = ii2_seg_host_blk_off(ctx, seg)) return rc0;
    info[0] = info[1] = info[2] = info[3] = 0;
    ii2_seg_store *store = seg->store.get();
    if (!store) return II2_OK;
    std::lock_guard<std::mutex> fg(store->form_mu);
    info[3] = store->form_bytes;
    if (seg->h_blk_off[list_idx] == seg->h_blk_off[list_idx + 1]) return II2_OK;       // (an empty list shares its block number with the next one)
    auto it = store->forms.find(seg->h_blk_off[list_idx]);
    if (it == store->forms.end() || !it->second.d_words) return II2_OK;
    info[0] = 1;
    info[1] = it->second.origin;
    info[2] = it->second.n_words;
    if (words) {
        if (cap < it->second.n_words) return fail(ctx, II2_ECAPACITY, "ii2_seg_dense_form: the form does not fit the buffer");
        HIP_TRY(ctx, hipMemcpyAsync(words, it->second.d_words, (size_t)it->second.n_words * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return II2_OK;
}

int ii2_seg_select(ii2_ctx *ctx, const ii2_seg *src, uint64_t n_out, const int64_t *src_list, ii2_seg **out) {
    if (!ctx || !src || !out || (n_out && !src_list) || src->device != ctx->device) return fail(ctx, II2_EINVAL, "ii2_seg_select: bad argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *out = nullptr;
    if (int rc0 = ii2_seg_host_blk_off(ctx, src)) return rc0;
    // selected lists must ascend, and only empty lists may be skipped between two selected ones
    std::vector<uint32_t> blk(n_out + 1, 0);
    int64_t prev = -1;
    uint32_t prev_end = 0;
    bool any = false;
    for (uint64_t i = 0; i < n_out; i++) {
        const int64_t j = src_list[i];
        if (j < 0) continue;
        if ((uint64_t)j >= src->n_lists || j <= prev) return fail(ctx, II2_EINVAL, "ii2_seg_select: list indices must ascend");
        const uint32_t b0 = src->h_blk_off[j], b1 = src->h_blk_off[j + 1];
        if (any && b0 != prev_end) return fail(ctx, II2_EINVAL, "ii2_seg_select: a non-empty list lies between two selected lists");
        prev = j;
        prev_end = b1;
        any = true;
    }
    uint32_t next = any ? prev_end : 0u;
    blk[n_out] = next;
    for (uint64_t i = n_out; i-- > 0;) {
        const int64_t j = src_list[i];
        if (j >= 0) next = src->h_blk_off[j];
        blk[i] = next;
    }
    std::unique_ptr<ii2_seg, void (*)(ii2_seg *)> seg(new (std::nothrow) ii2_seg(), seg_release);
    if (!seg) return II2_ENOMEM;
    seg->device = ctx->device;
    seg->born = ctx->stream;
    seg->store = src->store;
    seg->is_view = true;
    seg->d_skip = src->d_skip;
    seg->d_payload = src->d_payload;
    seg->n_lists = n_out;
    seg->n_blocks = src->n_blocks;
    seg->n_bytes = src->n_bytes;
    seg->n_postings = src->n_postings;      // upper bound: postings of unselected window lists are still counted
    if (dm_alloc((void **)&seg->d_blk_off, (n_out + 1) * sizeof(uint32_t)) != hipSuccess) return fail(ctx, II2_ENOMEM, "segment allocation failed");
    HIP_TRY(ctx, hipMemcpyAsync(seg->d_blk_off, blk.data(), (n_out + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    // the view's window of the store: blocks [blk[0], blk[n_out]) and the payload bytes between their skip entries
    ii2_skip w0, w1;
    std::memset(&w0, 0, sizeof w0); std::memset(&w1, 0, sizeof w1);
    if (n_out && blk[n_out] > blk[0]) {
        HIP_TRY(ctx, hipMemcpyAsync(&w0, src->d_skip + blk[0], sizeof w0, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&w1, src->d_skip + blk[n_out], sizeof w1, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (n_out && blk[n_out] > blk[0]) {
        seg->win_blocks = (uint64_t)blk[n_out] - blk[0];
        seg->win_bytes = std::max<uint64_t>((uint64_t)w1.byte_off - w0.byte_off, 1);
    } else {
        seg->win_blocks = 1; seg->win_bytes = 1;             // (nothing selected: a window of nothing; 0 would mean "the totals")
    }
    int rc = seg_finish(ctx, seg.get());
    if (rc) return rc;
    seg->born = nullptr;
    *out = seg.release();
    return II2_OK;
}

}  // extern "C"

// an empty segment shell with room for the given shape (ii2_seg_allgather fills it): ctx->mu held
int ii2_seg_alloc_internal(ii2_ctx *ctx, uint64_t n_lists, uint64_t n_postings, uint64_t n_blocks, uint64_t n_bytes, ii2_seg **out, bool with_meta) {
    std::unique_ptr<ii2_seg, void (*)(ii2_seg *)> seg(new (std::nothrow) ii2_seg(), seg_release);
    if (!seg) return II2_ENOMEM;
    seg->device = ctx->device;
    seg->born = ctx->stream;
    seg->n_lists = n_lists;
    seg->n_postings = n_postings;
    seg->n_blocks = n_blocks;
    seg->n_bytes = n_bytes;
    if (dm_alloc((void **)&seg->d_blk_off, (n_lists + 1) * sizeof(uint32_t)) != hipSuccess ||
        dm_alloc((void **)&seg->d_skip, (n_blocks + 1) * sizeof(ii2_skip)) != hipSuccess ||
        dm_alloc((void **)&seg->d_payload, n_bytes + 16) != hipSuccess)
        return fail(ctx, II2_ENOMEM, "segment allocation failed");
    if (with_meta) { if (int rcm = seg_alloc_meta(ctx, seg.get())) return rcm; }
    seg->born = nullptr;
    *out = seg.release();
    return II2_OK;
}

// the parts of a gathered segment (rank r: lists [lo[r], lo[r+1]), blocks [bo[r], bo[r+1]), bytes [qo[r], qo[r+1])) still
// number their blocks and bytes from 0: shift them, write the closing entries and derive the per-list arrays.  ctx->mu held
int ii2_seg_rebase_internal(ii2_ctx *ctx, ii2_seg *seg, int world, const uint64_t *lo, const uint64_t *bo, const uint64_t *qo) {
    hipStream_t st = ctx->stream;
    const bool have_meta = seg->d_blk_list != nullptr;           // the derived arrays travelled with the parts (ii2_seg_allgather)
    for (int r = 0; r < world; r++) {
        HIP_TRY(ctx, launch_seg_rebase(seg->d_blk_off + lo[r], lo[r + 1] - lo[r], (uint32_t)bo[r], seg->d_skip + bo[r], bo[r + 1] - bo[r], (uint32_t)qo[r],
                                       have_meta ? seg->d_blk_list + bo[r] : nullptr, (uint32_t)lo[r], st));
    }
    HIP_TRY(ctx, launch_seg_close(seg->d_blk_off + lo[world], (uint32_t)bo[world], seg->d_skip + bo[world], (uint32_t)qo[world], seg->d_payload + qo[world],
                                  have_meta ? seg->d_blk_list + bo[world] : nullptr, st));
    return seg_finish(ctx, seg, have_meta);                      // (one host wait: the segment is ready when this returns)
}

// host mirror of blk_off, fetched on first use (views built on the device do not have one)
int ii2_seg_host_blk_off(ii2_ctx *ctx, const ii2_seg *seg) {
    std::lock_guard<std::mutex> sg(seg->span_mu);
    if (seg->h_blk_off.size() == seg->n_lists + 1) return II2_OK;
    std::vector<uint32_t> h(seg->n_lists + 1);
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), seg->d_blk_off, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const_cast<ii2_seg *>(seg)->h_blk_off.swap(h);
    return II2_OK;
}

int ii2_seg_host_cnt(ii2_ctx *ctx, const ii2_seg *seg) {
    std::lock_guard<std::mutex> sg(seg->span_mu);
    if (seg->h_cnt.size() == seg->n_lists) return II2_OK;
    std::vector<uint32_t> h(seg->n_lists);
    if (seg->n_lists) {
        HIP_TRY(ctx, hipMemcpyAsync(h.data(), seg->d_cnt, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    const_cast<ii2_seg *>(seg)->h_cnt.swap(h);
    return II2_OK;
}

int ii2_seg_adopt_view(ii2_ctx *ctx, const ii2_seg *src, uint64_t n_out, uint32_t *d_blk_off, uint32_t *d_cnt, uint32_t *d_last_doc,
                       uint32_t *d_blk_list, ii2_seg **out) {
    ii2_seg *seg = new (std::nothrow) ii2_seg();
    if (!seg) {
        dm_free(d_blk_off); dm_free(d_cnt); dm_free(d_last_doc); dm_free(d_blk_list);
        return fail(ctx, II2_ENOMEM, "segment allocation failed");
    }
    seg->device = ctx->device;
    seg->born = ctx->stream;
    seg->store = src->store;
    seg->is_view = true;
    seg->d_skip = src->d_skip;
    seg->d_payload = src->d_payload;
    seg->n_lists = n_out;
    seg->n_blocks = src->n_blocks;
    seg->n_bytes = src->n_bytes;
    seg->n_postings = src->n_postings;      // upper bound, as for ii2_seg_select
    seg->d_blk_off = d_blk_off;
    seg->d_cnt = d_cnt;
    seg->d_last_doc = d_last_doc;
    seg->d_blk_list = d_blk_list;
    seg->born = nullptr;
    *out = seg;
    return II2_OK;
}

extern "C" {

void ii2_devmem_stats(uint64_t *live_bytes, uint64_t *idle_bytes) { dm_stats(live_bytes, idle_bytes); }

void ii2_seg_free(ii2_seg *seg) {
    if (!seg) return;
    // the caller guarantees no call that reads the segment is still running (as with any free); the arrays go back to the
    // size-class cache (devmem.cpp), which does not wait for the device
    (void)hipSetDevice(seg->device);
    seg_release(seg);
}

// ---- tombstones ---------------------------------------------------------------------------
int ii2_tomb_create(ii2_ctx *ctx, const uint32_t *removed, uint64_t n, int where, ii2_tomb **out) {
    if (!ctx || !out || (n && !removed)) return fail(ctx, II2_EINVAL, "ii2_tomb_create: bad argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *out = nullptr;
    const uint32_t *d_rem = removed;
    if (where == II2_HOST && n) {
        uint32_t *staged = (uint32_t *)ii2_pool_get(ctx, 1, n * sizeof(uint32_t));
        if (!staged) return fail(ctx, II2_ENOMEM, "tombstone staging allocation failed");
        HIP_TRY(ctx, hipMemcpyAsync(staged, removed, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        d_rem = staged;
    }
    uint32_t mx = 0;
    if (n) {
        uint32_t *d_mx = (uint32_t *)ctx->d_mail;
        HIP_TRY(ctx, hipMemsetAsync(d_mx, 0, sizeof(uint32_t), ctx->stream));
        HIP_TRY(ctx, launch_max_u32(d_rem, n, d_mx, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&mx, d_mx, sizeof mx, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    ii2_tomb *t = new (std::nothrow) ii2_tomb();
    if (!t) return II2_ENOMEM;
    t->device = ctx->device;
    t->n_words = n ? (uint64_t)(mx >> 5) + 1 : 0;
    // bitmap, then its summary (1 bit per (1 << TOMB_SUM_SHIFT) docs) in the same allocation
    const uint64_t words_padded = (t->n_words + TOMB_PAD_WORDS + 3) & ~3ull;      // (k_and2_words loads 16 bytes from the last word)
    const uint64_t n_sum = (t->n_words >> TOMB_SUM_SHIFT) + 2;
    if (ii2::dm_malloc_retry((void **)&t->d_words, (words_padded + n_sum) * sizeof(uint32_t)) != hipSuccess) {
        delete t;
        return fail(ctx, II2_ENOMEM, "tombstone bitmap allocation failed");
    }
    t->d_summary = t->d_words + words_padded;
    hipError_t e = hipMemsetAsync(t->d_words, 0, (words_padded + n_sum) * sizeof(uint32_t), ctx->stream);
    if (e == hipSuccess) e = launch_tomb_build(d_rem, n, t->d_words, t->n_words, t->d_summary, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(t->d_words);
        delete t;
        ctx->err = std::string("tombstone build: ") + hipGetErrorString(e);
        return II2_EHIP;
    }
    *out = t;
    return II2_OK;
}

void ii2_tomb_free(ii2_tomb *t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->d_words) (void)hipFree(t->d_words);
    delete t;
}

}  // extern "C"

// ---- look-back kernels ------------------------------------------------------------------------
// Look-back records for a launch of n_wg workgroups (lookback.h): a buffer of the context's own that only those kernels write,
// every word tagged with its launch's number - nothing to clear between launches (cleared when it grows or the numbers wrap).
// Kernels whose workgroups wait for lower-numbered workgroups of the SAME launch (lookback.h) must not share the GPU with
// another such launch: workgroups go to the eight XCDs round robin and every XCD starts its share in order, but the XCDs do not
// wait for each other - with two of these kernels from two contexts side by side, the workgroups of one can fill an XCD, spinning
// for a predecessor that sits in another XCD's queue behind the spinning workgroups of the other: each waits for a slot the
// other holds (seen: three contexts encoding merged segments at once under a tracer - every encoder ran out its seconds of
// bounded waits and handed over to the two-pass encoder).  The merge's tile kernel with direct placement waits too, but only for
// its scanner, workgroup 0 - the head of its XCD's queue: several of THEM side by side are safe (a freed slot goes to a
// scanner before it goes to any other workgroup of that kernel), one of them beside a look-back kernel is not.
// So, per device: a look-back kernel (exclusive = true) waits - on the GPU, not on the host - for every earlier kernel of
// either kind and every later one waits for it; tile kernels (exclusive = false) only wait for the last look-back kernel.
// Kernels without waits between workgroups run beside all of them as before.
// The order costs nothing while one context works alone: stream order already is an order, so nothing is recorded or waited for
// until a DIFFERENT stream comes along - which then records an event on the earlier stream itself (an event recorded late only
// covers more) and waits for that.  (Recording after every launch put a marker between back-to-back queries of one context: 41 ->
// 46 us per two-list AND.)
namespace {
struct LbChain {
    hipEvent_t ev_x = nullptr;              // the last exclusive kernel: recorded here (x_recorded), or still only in its stream's order (x_stream)
    bool x_recorded = false;
    hipStream_t x_stream = nullptr;         // stream of the last exclusive kernel while the event is not recorded yet
    hipStream_t x_owner = nullptr;          // ... and once it is (that stream needs no wait)
    hipEvent_t ev_s[16] = {};               // the shared kernels since then: one stream each
    hipStream_t s_stream[16] = {};
    unsigned n_s = 0;
};
std::mutex g_lb_mu;
LbChain g_lb[64];
}  // namespace
int ii2_lookback_launch(ii2_ctx *ctx, bool exclusive, const std::function<hipError_t()> &launch) {
    const int dev = ctx->device;
    if (dev < 0 || dev >= 64) return fail(ctx, II2_EINVAL, "device number out of range");
    if (ctx->opt_debug_no_chain) { HIP_TRY(ctx, launch()); return II2_OK; }      // (experiments: what happens without the order)
    std::lock_guard<std::mutex> g(g_lb_mu);
    LbChain &c = g_lb[dev];
    hipStream_t me = ctx->stream;
    if (!c.ev_x) {
        HIP_TRY(ctx, hipEventCreateWithFlags(&c.ev_x, hipEventDisableTiming));
        for (int i = 0; i < 16; i++) HIP_TRY(ctx, hipEventCreateWithFlags(&c.ev_s[i], hipEventDisableTiming));
    }
    // behind the last exclusive kernel
    if (c.x_stream && c.x_stream != me) {
        HIP_TRY(ctx, hipEventRecord(c.ev_x, c.x_stream));
        c.x_recorded = true; c.x_owner = c.x_stream; c.x_stream = nullptr;
    }
    if (c.x_recorded && c.x_owner != me) { HIP_TRY(ctx, hipStreamWaitEvent(me, c.ev_x, 0)); ctx->lb_waits++; }
    if (exclusive) {
        // ... and behind every shared kernel since then
        for (unsigned i = 0; i < c.n_s; i++) {
            if (c.s_stream[i] == me) continue;
            HIP_TRY(ctx, hipEventRecord(c.ev_s[i], c.s_stream[i]));
            HIP_TRY(ctx, hipStreamWaitEvent(me, c.ev_s[i], 0));
            ctx->lb_waits++;
        }
        c.n_s = 0;
        HIP_TRY(ctx, launch());
        c.x_stream = me; c.x_recorded = false; c.x_owner = nullptr;
    } else {
        bool known = false;
        for (unsigned i = 0; i < c.n_s; i++) known |= c.s_stream[i] == me;
        if (!known && c.n_s == 16u) {          // (more than 16 streams with a shared kernel in flight: this one queues behind the first)
            HIP_TRY(ctx, hipEventRecord(c.ev_s[0], c.s_stream[0]));
            HIP_TRY(ctx, hipStreamWaitEvent(me, c.ev_s[0], 0));
            ctx->lb_waits++;
            c.s_stream[0] = me;
            known = true;
        }
        HIP_TRY(ctx, launch());
        if (!known) c.s_stream[c.n_s++] = me;
    }
    return II2_OK;
}
// a context goes away (its stream has been waited for): nothing of it is left to wait for
void ii2_lookback_forget(ii2_ctx *ctx) {
    if (ctx->device < 0 || ctx->device >= 64) return;
    std::lock_guard<std::mutex> g(g_lb_mu);
    LbChain &c = g_lb[ctx->device];
    if (c.x_stream == ctx->stream) c.x_stream = nullptr;
    if (c.x_owner == ctx->stream) c.x_owner = nullptr;          // (the recorded event stays valid: it is the chain's own)
    unsigned k = 0;
    for (unsigned i = 0; i < c.n_s; i++)
        if (c.s_stream[i] != ctx->stream) c.s_stream[k++] = c.s_stream[i];
    c.n_s = k;
}

// The error word holds the epoch of the LAST launch that gave up, and ii2_ctx_sync looks at it for the asynchronous launches
// since the previous sync (lb_pending .. lb_epoch).  A synchronous call's own launch may overwrite it, and new records clear
// it: before either, the word is copied into the mailbox behind those launches (lb_note_pending), and once the stream has
// passed the copy (lb_fold_pending) a give-up among them is kept for ii2_ctx_sync.  A synchronous call's own give-up is
// handled by that call (repeated, exact) and never reported there.
void lb_fold_pending(ii2_ctx *ctx) {
    if (!ctx->lb_snap_first) return;
    const uint64_t e = ctx->h_mail[II2_MAIL_LB_PENDING];
    if (e >= ctx->lb_snap_first && e <= ctx->lb_snap_last) ctx->lb_async_failed = true;
    ctx->lb_snap_first = ctx->lb_snap_last = 0;
}
int lb_note_pending(ii2_ctx *ctx) {
    if (!ctx->lb_pending || !ctx->d_lb) return II2_OK;
    if (ctx->lb_snap_first) {                       // (an earlier copy nobody has looked at: only after a call that failed)
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        lb_fold_pending(ctx);
    }
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_mail + II2_MAIL_LB_PENDING, ctx->d_lb, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    ctx->lb_snap_first = ctx->lb_pending;
    ctx->lb_snap_last = ctx->lb_epoch;
    ctx->lb_pending = 0;
    return II2_OK;
}

int ii2_lookback_prepare(ii2_ctx *ctx, size_t n_wg, ii2::LookBack *lb) {
    hipStream_t st = ctx->stream;
    if (n_wg > ctx->lb_cap || ctx->lb_epoch >= (1u << 24) - 1u) {
        if (int rcn = lb_note_pending(ctx)) return rcn;       // (the records are about to be cleared)
        HIP_TRY(ctx, hipStreamSynchronize(st));
        lb_fold_pending(ctx);
        if (n_wg > ctx->lb_cap) {
            if (ctx->d_lb) (void)hipFree(ctx->d_lb);
            ctx->d_lb = nullptr;
            ctx->lb_cap = 0;
            const size_t cap_wg = std::max<size_t>(4096, n_wg + n_wg / 4);
            if (ii2::dm_malloc_retry((void **)&ctx->d_lb, (8 + cap_wg + 2 * ((cap_wg + 63) / 64)) * sizeof(unsigned long long)) != hipSuccess)
                return fail(ctx, II2_ENOMEM, "look-back records allocation failed");
            ctx->lb_cap = cap_wg;
        }
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_lb, 0, (8 + ctx->lb_cap + 2 * ((ctx->lb_cap + 63) / 64)) * sizeof(unsigned long long), st));
        ctx->lb_epoch = 0;
        ctx->lb_pending = 0;
    }
    lb->err = ctx->d_lb;
    lb->agg = ctx->d_lb + 8;
    lb->grp = ctx->d_lb + 8 + ctx->lb_cap;
    lb->epoch = ++ctx->lb_epoch;
    lb->spin = 0;
    if (!ctx->lb_pending) ctx->lb_pending = lb->epoch;
    return II2_OK;
}

extern "C" {

// The protocol alone, on this context's records and epoch (ii2.h; lookback_check.hip): prepared and launched like the kernels
// that use it, so what it leaves in the records and what they leave is the same state.
int ii2_lookback_check(ii2_ctx *ctx, uint32_t n_wg, uint32_t g_base, const uint64_t *amount, uint32_t spin, const uint8_t *seed_state,
                       const uint64_t *seed_value, const uint16_t *delay, uint64_t *out_prefix, uint32_t *out_state, uint32_t *out_walk,
                       uint32_t *out_polls, uint64_t *out_agg, uint64_t *out_grp, uint64_t *out_info) {
    if (!ctx) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    if (n_wg == 0 || n_wg > II2_LB_CHECK_MAX_WG || g_base >= n_wg || g_base % LB_GROUP != 0 || !amount || spin == 0 || spin > II2_LB_CHECK_MAX_SPIN ||
        !out_prefix || !out_state || !out_walk || !out_polls || !out_agg || !out_grp || !out_info || (g_base && (!seed_state || !seed_value)))
        return fail(ctx, II2_EINVAL, "ii2_lookback_check: bad argument");
    const uint32_t n_launched = n_wg - g_base, grp_base = g_base / LB_GROUP, n_grp = (n_wg + LB_GROUP - 1u) / LB_GROUP - grp_base;
    const size_t n_seed = (size_t)g_base + 2u * grp_base;
    unsigned long long total = 0;
    for (uint32_t i = 0; i < n_wg; i++) {
        if (amount[i] > LB_VALUE_MASK || (total += amount[i]) > LB_VALUE_MASK) return fail(ctx, II2_EINVAL, "ii2_lookback_check: the amounts and their sum are below 2^40");
        if (delay && delay[i] > II2_LB_CHECK_MAX_DELAY) return fail(ctx, II2_EINVAL, "ii2_lookback_check: a delay is at most II2_LB_CHECK_MAX_DELAY");
    }
    for (size_t i = 0; i < n_seed; i++)
        if (seed_state[i] > II2_LB_SEED_LATER || seed_value[i] > LB_VALUE_MASK) return fail(ctx, II2_EINVAL, "ii2_lookback_check: bad seed");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rcw = ii2_ws_reserve(ctx, align_up((size_t)n_wg * sizeof(uint64_t)) + align_up((size_t)n_wg * sizeof(uint16_t)) +
                                          align_up((size_t)n_launched * sizeof(uint64_t)) + 3 * align_up((size_t)n_launched * sizeof(uint32_t)) + 4096))
        return rcw;
    LbCheckParams p;
    unsigned long long *d_amount = ws_take<unsigned long long>(ctx, n_wg);
    uint16_t *d_delay = ws_take<uint16_t>(ctx, n_wg);
    p.n_wg = n_wg; p.g_base = g_base; p.amount = d_amount; p.delay = delay ? d_delay : nullptr;
    p.prefix = ws_take<unsigned long long>(ctx, n_launched);
    p.state = ws_take<uint32_t>(ctx, n_launched);
    p.walk = ws_take<uint32_t>(ctx, n_launched);
    p.polls = ws_take<uint32_t>(ctx, n_launched);
    if (int rcn = lb_note_pending(ctx)) return rcn;       // (the give-ups of asynchronous launches before this one stay reported)
    if (int rcl = ii2_lookback_prepare(ctx, n_wg, &p.lb)) return rcl;
    ctx->lb_pending = 0;                           // (this call reports its own give-up, below)
    p.lb.spin = spin;
    // the records of the workgroups and groups before the launched ones, as the caller wants them found
    std::vector<unsigned long long> seed(n_seed);
    for (size_t i = 0; i < n_seed; i++) {
        const uint32_t tag = seed_state[i] == II2_LB_SEED_READY ? p.lb.epoch : seed_state[i] == II2_LB_SEED_STALE ? p.lb.epoch - 1u : p.lb.epoch + 1u;
        seed[i] = seed_state[i] == II2_LB_SEED_MISSING ? 0ull : ((unsigned long long)(tag & LB_EPOCH_MAX) << LB_VALUE_BITS) | seed_value[i];
    }
    HIP_TRY(ctx, hipMemcpyAsync(d_amount, amount, (size_t)n_wg * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (delay) HIP_TRY(ctx, hipMemcpyAsync(d_delay, delay, (size_t)n_wg * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    if (g_base) {
        HIP_TRY(ctx, hipMemcpyAsync(p.lb.agg, seed.data(), (size_t)g_base * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(p.lb.grp, seed.data() + g_base, 2 * (size_t)grp_base * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    }
    if (int rcq = ii2_lookback_launch(ctx, true, [&] { return launch_lb_check(p, st); })) return rcq;
    uint64_t err_word = 0;
    HIP_TRY(ctx, hipMemcpyAsync(out_prefix, p.prefix, (size_t)n_launched * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out_state, p.state, (size_t)n_launched * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out_walk, p.walk, (size_t)n_launched * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out_polls, p.polls, (size_t)n_launched * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out_agg, p.lb.agg + g_base, (size_t)n_launched * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out_grp, p.lb.grp + 2 * (size_t)grp_base, 2 * (size_t)n_grp * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(&err_word, p.lb.err, sizeof err_word, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    lb_fold_pending(ctx);
    out_info[0] = p.lb.epoch;
    out_info[1] = err_word;
    out_info[2] = ctx->lb_cap;
    return II2_OK;
}

int ii2_selftest(ii2_ctx *ctx) {
    if (!ctx) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ii2_ws_reserve(ctx, SELFTEST_SCRATCH + 4096);
    if (rc) return rc;
    uint8_t *scratch = ws_take<uint8_t>(ctx, SELFTEST_SCRATCH);
    uint32_t *d_fail = (uint32_t *)ctx->d_mail;
    HIP_TRY(ctx, hipMemsetAsync(d_fail, 0, sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, launch_selftest(d_fail, scratch, ctx->stream));
    uint32_t f = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&f, d_fail, sizeof f, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (f) {
        char msg[96];
        std::snprintf(msg, sizeof msg, "device self-test failed, mask 0x%x (1=scan 2=decode 4=count)", f);
        ctx->err = msg;
        return (int)f;
    }
    return II2_OK;
}

int ii2_ctx_counters(ii2_ctx *ctx, uint64_t *out, uint32_t n) {
    if (!ctx || !out) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    if (n > 0) out[0] = ctx->merge_fallbacks;
    if (n > 1) out[1] = ctx->lb_fallbacks;
    if (n > 2) out[2] = ctx->comm_syncs;
    if (n > 3) out[3] = ctx->lb_waits;
    return II2_OK;
}

// the names of ii2::Path, in the enum's order
static const char *const PATH_NAMES[] = {
    "and.small", "and.and2_fused", "and.and2_split", "and.dense2", "and.dense3", "and.dense4",
    "and.tiles_pair", "and.tiles", "and.tiles_wide", "and.tiles_sub", "and.tiles_wide_sub",
    "or.small", "or.rank", "or.stream2", "or.stream3", "or.stream4", "or.tiles", "or.tiles_wide", "or.merge",
    "or.many", "or.many_window", "or.many_count_first",
    "ir.handoff", "ir.groups", "ir.probe", "ir.mark", "ir.probe_drop", "ir.mark_drop",
    "andnot.small", "andnot.general",
    "batch.tiny", "batch.small", "batch.single", "batch.pack",
    "gbatch.tiny", "gbatch.small", "gbatch.single", "gbatch.pack",
    "span.fetch", "span.bounds",
};
static_assert(sizeof PATH_NAMES / sizeof PATH_NAMES[0] == ii2::P_COUNT, "one name per ii2::Path");

int ii2_ctx_paths(ii2_ctx *ctx, uint64_t *out, uint32_t n) {
    if (!ctx || (!out && n)) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    for (uint32_t i = 0; i < n && i < ii2::P_COUNT; i++) out[i] = ctx->paths[i];
    return (int)ii2::P_COUNT;
}

const char *ii2_path_name(uint32_t i) { return i < ii2::P_COUNT ? PATH_NAMES[i] : nullptr; }

// the names of ii2::MergeEvent, in the enum's order
static const char *const MERGE_EVENT_NAMES[] = {"batch_redo", "range_overfull", "range_bucket_overflow", "leaf_bitmap", "leaf_sorted"};
static_assert(sizeof MERGE_EVENT_NAMES / sizeof MERGE_EVENT_NAMES[0] == ii2::ME_COUNT, "one name per ii2::MergeEvent");

int ii2_merge_events(ii2_ctx *ctx, uint64_t *out, uint32_t n) {
    if (!ctx || (!out && n)) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    unsigned long long ev[ii2::ME_COUNT];
    HIP_TRY(ctx, hipMemcpyAsync(ev, ctx->d_merge_events, sizeof ev, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t i = 0; i < n && i < ii2::ME_COUNT; i++) out[i] = ev[i];
    return (int)ii2::ME_COUNT;
}

const char *ii2_merge_event_name(uint32_t i) { return i < ii2::ME_COUNT ? MERGE_EVENT_NAMES[i] : nullptr; }

int ii2_debug_read(ii2_ctx *ctx, uint64_t *out, uint64_t n_words) {
    if (!ctx || !out || !ctx->d_debug) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    const uint64_t have = (uint64_t)2048 * 8;
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_debug, std::min(n_words, have) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return II2_OK;
}

int ii2_set_option(ii2_ctx *ctx, const char *name, int64_t value) {
    if (!ctx || !name) return II2_EINVAL;
    std::lock_guard<std::mutex> g(ctx->mu);
    const std::string k(name);
    if (k == "intersect.g") ctx->opt_intersect_g = value;
    else if (k == "intersect.wgs") ctx->opt_intersect_wgs = value;
    else if (k == "merge.large_tile") ctx->opt_merge_large_tile = value;
    else if (k == "merge.bitmap_tiles") ctx->opt_merge_bitmap = value;
    else if (k == "debug.merge_skip") ctx->opt_merge_skip = value;
    else if (k == "merge.direct") ctx->opt_merge_direct = value;
    else if (k == "merge.spin") ctx->opt_merge_spin = value;
    else if (k == "debug.stamps") ctx->opt_debug_stamps = value;
    else if (k == "merge.alone") ctx->opt_merge_alone = value;
    else if (k == "debug.no_chain") ctx->opt_debug_no_chain = value;
    else if (k == "debug.lb_epoch") {       // tests: the number of the last look-back launch (the next one takes value + 1, or wraps)
        if (value < 0 || value > (int64_t)LB_EPOCH_MAX) return fail(ctx, II2_EINVAL, "debug.lb_epoch: 0 .. 2^24 - 1");
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        ctx->lb_epoch = (uint32_t)value;
    }
    else if (k == "profile.events") ctx->opt_profile_events = value;
    else if (k == "intersect.bitmap") ctx->opt_intersect_bitmap = value;
    else if (k == "union.dense") ctx->opt_union_dense = value;
    else if (k == "union.stream") ctx->opt_union_stream = value;
    else if (k == "setop.small") ctx->opt_small_setop = value;
    else if (k == "union.rank") ctx->opt_union_rank = value;
    else if (k == "batch.small") ctx->opt_batch_small = value;
    else if (k == "batch.tiny") ctx->opt_batch_tiny = value;
    else if (k == "batch.groups") ctx->opt_batch_groups = value;
    else if (k == "batch.topk") ctx->opt_batch_topk = value;
    else if (k == "batch.explain") ctx->opt_batch_explain = value;
    else if (k == "union.many") ctx->opt_union_many = value;
    else if (k == "union.many_window_log2") ctx->opt_union_many_window_log2 = value;
    else if (k == "debug.union_many_no_atomics") ctx->opt_union_many_no_atomics = value;
    else if (k == "count.summary_skip") ctx->opt_count_summary_skip = value;
    else if (k == "hist.per_wave") ctx->opt_hist_per_wave = value;
    else if (k == "hist.whole") ctx->opt_hist_whole = value;
    else if (k == "match.stage") ctx->opt_match_stage = value;
    else if (k == "fuzzy.stage") ctx->opt_fuzzy_stage = value;
    else if (k == "fuzzy.wide") ctx->opt_fuzzy_wide = value;
    else if (k == "regex.stage") ctx->opt_regex_stage = value;
    else if (k == "intersect.ranges") ctx->opt_intersect_ranges = value;
    else if (k == "intersect.ranges_mark") ctx->opt_ir_mark = value;
    else if (k == "andnot.small") ctx->opt_andnot_small = value;
    else if (k == "atleast.small") ctx->opt_atleast_small = value;
    else if (k == "atleast.handoff") ctx->opt_atleast_handoff = value;
    else if (k == "topk.late") ctx->opt_topk_late = value;
    else if (k == "union.sparsity") ctx->opt_union_sparsity = value > 0 ? value : 2048;
    else if (k == "intersect.map_docs") ctx->opt_intersect_map_docs = value;
    else if (k == "intersect.dense") ctx->opt_intersect_dense = value;
    else if (k == "intersect.dense_bpw") ctx->opt_dense_bpw = value;
    else if (k == "intersect.subtiles") ctx->opt_intersect_subtiles = value;
    else if (k == "intersect.submax") ctx->opt_intersect_submax = value;
    else if (k == "intersect.and2") ctx->opt_intersect_and2 = value;      // 0: n-list kernel, 1: one launch (look-back), 2: two kernels
    else if (k == "intersect.and2_spin") ctx->opt_and2_spin = value;
    else if (k == "intersect.and2_tiles") ctx->opt_and2_tiles = value;    // 0: auto (setop.cpp and2_tiles_pick), 1, 2: tiles per wave where the longer list has a dense form
    else if (k == "intersect.and2_slots") ctx->opt_and2_slots = value;    // auto's "workgroups the device holds at once" (0: asked of the runtime)
    else if (k == "intersect.and2_words") ctx->opt_and2_words = value;    // two dense lists, both as cached bitmaps, ANDed word by word: 0 never, 1 by the rule (setop.cpp and2_words_pick), 2 always (tests)
    else if (k == "intersect.and2_words_store") ctx->opt_and2_words_store = value;    // ... its id stores: 0 plain, 1 (default) write-through and 16-byte aligned
    else if (k == "intersect.and2_words_order") ctx->opt_and2_words_order = value;    // ... 0 (default) both chunks staged before the first store, 1 (measurements) chunk 0's stores first
    else if (k == "intersect.and2_words_min") ctx->opt_and2_words_min = value;    // the rule's "blocks the shorter list holds at least" (0: CUs x the runtime's occupancy answer x 16)
    else if (k == "intersect.dense_form") ctx->opt_dense_form = value;    // 0: never, 1: where the form is <= half the list's payload, 2: always (tests)
    else if (k == "encode.stream") ctx->opt_encode_stream = value;        // 1: one-pass encoder behind a merge (default), 0: two-pass, -1: forced fallback (tests)
    else return fail(ctx, II2_EINVAL, "unknown option");
    return II2_OK;
}

}  // extern "C"
