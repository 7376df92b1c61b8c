// dict_find.hip — term and prefix lookup in resident dictionaries, hand-written: the step in front of every range entry point.
//
// Replaces the bisections that turn a query's terms into list indices, one per (term, segment): the FST lookups behind
// InvertedIndex.Intersect / PrefixSearch (inverted_index.go:274-292), in bytes.Compare order (file/types.go:24-26).  Many
// independent probes against k dictionaries that live in HBM (ii2_dict, align.hip); the answer of probe p in dictionary s is
// entry p * k + s, so the k ranges of one term are adjacent - one group of the range entry points.
//
// Method: one thread per (probe, dictionary), a workgroup takes consecutive probes of ONE dictionary, so the top levels of its
// bisections read the same cache lines.  The probe's 8-byte key is formed from its bytes; the bisection runs in global memory over
// the dictionary's keys and goes to the bytes on ties (term_device.h).  A form that first bracketed every probe in an LDS sample
// of 2048 of the dictionary's keys was measured and was not faster.  No workgroup waits for another; the only
// atomics are the error word and the count of non-empty ranges.
#include <cstring>
#include <vector>

#include "internal.h"
#include "term_device.h"

namespace ii2 {

constexpr uint32_t DF_THREADS = 256;

struct FindDicts {
    const uint64_t *key[MAX_LISTS];
    const uint64_t *off[MAX_LISTS];
    const uint8_t *bytes[MAX_LISTS];
    uint32_t n[MAX_LISTS];
    uint32_t k;
};

// probe offsets ascending from 0 (bad |= 1), flags 0 / 1 (bad |= 2): arrays that live on the device are checked there
__global__ void k_probe_check(const uint64_t *__restrict__ off, const uint8_t *__restrict__ prefix, uint64_t n, uint32_t *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (off[i + 1] < off[i] || (i == 0 && off[0] != 0)) atomicOr(bad, 1u);
    if (prefix && prefix[i] > 1u) atomicOr(bad, 2u);
}

// workgroup (x, s): probes [x * DF_THREADS, (x + 1) * DF_THREADS) in dictionary s.  *bad != 0 (k_probe_check, same stream): nothing is read or written.
__global__ __launch_bounds__(DF_THREADS) void k_dict_find(FindDicts d, uint64_t n_probes, const uint8_t *__restrict__ probe_bytes,
                                                          const uint64_t *__restrict__ probe_off, const uint8_t *__restrict__ probe_prefix,
                                                          const uint32_t *__restrict__ bad, uint64_t *__restrict__ list_first, uint64_t *__restrict__ list_end,
                                                          unsigned long long *__restrict__ n_found) {
    __shared__ uint32_t wave_found[DF_THREADS / 64];
    if (*bad) return;
    const uint32_t s = blockIdx.y, n = d.n[s];
    const TermDict td{d.key[s], d.off[s], d.bytes[s]};
    const uint64_t p = (uint64_t)blockIdx.x * DF_THREADS + threadIdx.x;
    uint32_t mine = 0;
    if (p < n_probes) {
        const uint64_t b = probe_off[p], len = probe_off[p + 1] - b;
        const TermRef x{term_key(probe_bytes + b, len), probe_bytes + b, len};
        uint32_t first, end;
        term_find(td, n, x, probe_prefix && probe_prefix[p], &first, &end);
        list_first[p * d.k + s] = first;
        list_end[p * d.k + s] = end;
        mine = end > first ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
    if ((threadIdx.x & 63u) == 0u) wave_found[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
        for (uint32_t w = 0; w < DF_THREADS / 64; w++) all += wave_found[w];
        if (all) atomicAdd(n_found, (unsigned long long)all);
    }
}

}  // namespace ii2

using namespace ii2;

extern "C" {

int ii2_dict_find(ii2_ctx *ctx, uint32_t k, const ii2_dict *const *dicts, uint64_t n_probes, const uint8_t *probe_bytes, const uint64_t *probe_off,
                  const uint8_t *probe_prefix, int where, uint64_t *list_first, uint64_t *list_end, uint64_t *n_found) {
    if (!ctx || !dicts || k == 0 || k > II2_MAX_LISTS || (where != II2_HOST && where != II2_DEVICE))
        return fail(ctx, II2_EINVAL, "ii2_dict_find: bad argument");
    if (n_probes && (!probe_bytes || !probe_off || !list_first || !list_end)) return fail(ctx, II2_EINVAL, "ii2_dict_find: an array is NULL");
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    FindDicts fd;
    std::memset(&fd, 0, sizeof fd);
    fd.k = k;
    for (uint32_t s = 0; s < k; s++) {
        if (!dicts[s] || dicts[s]->device != ctx->device) return fail(ctx, II2_EINVAL, "ii2_dict_find: a dictionary is NULL or lives on another device");
        fd.key[s] = dicts[s]->d_key; fd.off[s] = dicts[s]->d_off; fd.bytes[s] = dicts[s]->d_bytes;
        fd.n[s] = (uint32_t)dicts[s]->n;
    }
    if (n_probes > 0xFFFFFFFFull / k) return fail(ctx, II2_ERANGE, "ii2_dict_find: 2^32 or more (probe, dictionary) pairs");
    if (n_probes == 0) {
        if (n_found) *n_found = 0;
        return II2_OK;
    }
    if (where == II2_HOST) {
        if (probe_off[0] != 0) return fail(ctx, II2_EINVAL, "ii2_dict_find: probe_off must start at 0 and be non-decreasing");
        for (uint64_t p = 0; p < n_probes; p++) {
            if (probe_off[p + 1] < probe_off[p]) return fail(ctx, II2_EINVAL, "ii2_dict_find: probe_off must start at 0 and be non-decreasing");
            if (probe_prefix && probe_prefix[p] > 1) return fail(ctx, II2_EINVAL, "ii2_dict_find: a prefix flag is neither 0 nor 1");
        }
    }
    const uint64_t n_out = n_probes * k;
    hipStream_t st = ctx->stream;
    const uint8_t *d_bytes = probe_bytes, *d_prefix = probe_prefix;
    const uint64_t *d_off = probe_off;
    uint64_t *d_first = list_first, *d_end = list_end;
    unsigned long long *d_found = (unsigned long long *)ctx->d_mail;      // [0] non-empty ranges, [1] the probes' error word
    uint32_t *d_bad = (uint32_t *)(ctx->d_mail + 1);
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_mail, 0, 2 * sizeof(uint64_t), st));
    if (where == II2_HOST) {
        const uint64_t nb = probe_off[n_probes];
        int rc = ii2_ws_reserve(ctx, align_up(nb + 16) + align_up((n_probes + 1) * sizeof(uint64_t)) + align_up(n_probes) + 2 * align_up(n_out * sizeof(uint64_t)));
        if (rc) return rc;
        uint8_t *w_bytes = ws_take<uint8_t>(ctx, nb + 16);
        uint64_t *w_off = ws_take<uint64_t>(ctx, n_probes + 1);
        uint8_t *w_prefix = ws_take<uint8_t>(ctx, n_probes);
        d_first = ws_take<uint64_t>(ctx, n_out);
        d_end = ws_take<uint64_t>(ctx, n_out);
        if (nb) HIP_TRY(ctx, hipMemcpyAsync(w_bytes, probe_bytes, nb, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(w_off, probe_off, (n_probes + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        if (probe_prefix) HIP_TRY(ctx, hipMemcpyAsync(w_prefix, probe_prefix, n_probes, hipMemcpyHostToDevice, st));
        d_bytes = w_bytes;
        d_off = w_off;
        d_prefix = probe_prefix ? w_prefix : nullptr;
    } else {
        hipLaunchKernelGGL(k_probe_check, dim3((unsigned)((n_probes + 255) / 256)), dim3(256), 0, st, d_off, d_prefix, n_probes, d_bad);
    }
    hipLaunchKernelGGL(k_dict_find, dim3((unsigned)((n_probes + DF_THREADS - 1) / DF_THREADS), k), dim3(DF_THREADS), 0, st, fd, n_probes, d_bytes, d_off, d_prefix,
                       (const uint32_t *)d_bad, d_first, d_end, d_found);
    HIP_TRY(ctx, hipGetLastError());
    uint64_t mail[2] = {0, 0};
    if (where == II2_HOST) {
        HIP_TRY(ctx, hipMemcpyAsync(list_first, d_first, n_out * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(list_end, d_end, n_out * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(ctx, hipMemcpyAsync(mail, ctx->d_mail, sizeof mail, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                       // the one wait
    const uint32_t bad = (uint32_t)mail[1];
    if (bad & 1u) return fail(ctx, II2_EINVAL, "ii2_dict_find: probe_off must start at 0 and be non-decreasing");
    if (bad & 2u) return fail(ctx, II2_EINVAL, "ii2_dict_find: a prefix flag is neither 0 nor 1");
    if (n_found) *n_found = mail[0];
    return II2_OK;
}

// host only: one probe against one host dictionary, by the functions k_dict_find runs - the keys, the bisection with the full
// comparison and the prefix run's end
int ii2_term_bounds(const uint8_t *term_bytes, const uint64_t *term_off, uint64_t n_terms, const uint8_t *probe, uint64_t probe_len, int prefix,
                    uint64_t *first, uint64_t *end) {
    if (!first || !end || (n_terms && !term_off) || (probe_len && !probe) || (prefix != 0 && prefix != 1)) return II2_EINVAL;
    if (n_terms >= (1ull << 31)) return II2_ERANGE;
    if (n_terms && term_off[0] != 0) return II2_EINVAL;
    for (uint64_t i = 0; i < n_terms; i++)
        if (term_off[i + 1] < term_off[i]) return II2_EINVAL;
    if (n_terms && term_off[n_terms] && !term_bytes) return II2_EINVAL;
    const uint32_t n = (uint32_t)n_terms;
    std::vector<uint64_t> key(n);
    for (uint32_t i = 0; i < n; i++) key[i] = term_key(term_bytes + term_off[i], term_off[i + 1] - term_off[i]);
    const TermDict td{key.data(), term_off, term_bytes};
    const TermRef x{term_key(probe, probe_len), probe, probe_len};
    uint32_t f, e;
    term_find(td, n, x, prefix != 0, &f, &e);
    *first = f;
    *end = e;
    return II2_OK;
}

}  // extern "C"
