// dict_build.hip — ii2_dict_build: a resident, sorted, duplicate-free dictionary from raw term bytes (gfx950, wave64).
//
// The step between documents and ii2_seg_build: what Shard.PutBatch's host code does with a std::sort, a std::unique and one
// string bisection per term occurrence (order = file.CompareTermValues = bytes.Compare, file/types.go:24-26).  n terms in any
// order, repeats allowed, go in; an ii2_dict like the one ii2_dict_create makes from sorted(set(terms)) comes out, and with it
// the index of every input term in it - the list_id array of ii2_seg_build.
//
// bytes.Compare order is the order of the tuple (chunk 0, chunk 1, ..., chunk C - 1, length): chunk c = bytes [8c, 8c + 8)
// big-endian, zero padded (term_chunk, term_device.h), C = ceil(max_len / 8).  So the sort is a stable least-significant-digit
// radix sort of (64-bit key, 32-bit input index) pairs, 8-bit digits, the passes of radix_device.h: the length first, then
// the chunks C - 1 down to 0, and ONLY THE BYTES THAT CAN DIFFER get a pass.  NO WORKGROUP EVER WAITS FOR ANOTHER.
//
//   k_db_plan      a thread per term, a few workgroups per CU striding over them: the offsets are checked (ascending from 0,
//                  inside [0, term_off[n]], no term above II2_DICT_BUILD_MAX_TERM - a term that fails is not read), and min /
//                  max / OR / AND of the lengths and, per chunk, OR and AND of the keys of the terms that reach into it are
//                  reduced - in the wave first, then in the workgroup, then one atomic per workgroup and word.  One readback
//                  (wait 1); db_passes turns the words into the passes.
//   k_db_gather    key[i] = the length, or chunk c, of term idx[i] in the current order (the first one also sets idx[i] = i)
//   k_db_hist / k_db_scatter   one pass over the pairs.  The scatter keeps only keys and ranks in registers: the indices are
//                  reloaded, coalesced, when the tile is staged through LDS (32 KB of keys + 16 KB of indices).
//   k_db_heads     head flag = the term differs from its predecessor in sorted order (term_cmp, the chunk-0 keys first; a
//                  wave's first lane reads its predecessor from global memory).  Run once to count the heads per tile and sum
//                  their lengths (readback: wait 2, sizes the dictionary), and - after a scan - again: every sorted position
//                  gets the rank of its run's head (term_id[idx[i]] = rank), every head its length, key and source index.
//   k_db_bytes     the dictionary's bytes, gathered from the source terms at the scanned lengths.
// The end is wait 3.
#include <algorithm>
#include <cstring>
#include <memory>

#include "radix_device.h"
#include "term_device.h"

namespace ii2 {

constexpr uint32_t DB_CHUNKS = II2_DICT_BUILD_MAX_TERM / 8u;      // 32 chunks of 8 bytes at most
constexpr uint32_t DB_LEN = 0xFFFFFFFFu;                           // k_db_gather: the length instead of a chunk
// control words of one call in the context's mailbox (u64 each): [0, DB_CTL_ONES) start as 0, [DB_CTL_ONES, DB_CTL_WORDS) as all ones
constexpr uint32_t DB_CTL_BAD = 0, DB_CTL_MAX_LEN = 1, DB_CTL_LEN_OR = 2, DB_CTL_BYTES = 3, DB_CTL_OR = 4, DB_CTL_ONES = DB_CTL_OR + DB_CHUNKS,
                   DB_CTL_MIN_LEN = DB_CTL_ONES, DB_CTL_LEN_AND = DB_CTL_ONES + 1, DB_CTL_AND = DB_CTL_ONES + 2, DB_CTL_WORDS = DB_CTL_AND + DB_CHUNKS;
static_assert(II2_MAIL_DICT_BUILD + DB_CTL_WORDS + 1 <= II2_MAIL_COUNT, "the control words overlap the result count");

// what the terms' reduction leaves: the words of k_db_plan, or of the host loop of ii2_dict_build_plan
struct DbPlan {
    uint64_t min_len, max_len, len_or, len_and;
    uint64_t ch_or[DB_CHUNKS], ch_and[DB_CHUNKS];      // over the terms that reach into the chunk
};

__host__ __device__ __forceinline__ uint32_t db_chunks(uint64_t len) { return (uint32_t)((len + 7u) / 8u); }

// The passes: byte position p of the terms gets one where some two terms can differ there - OR & ~AND of its chunk, the AND
// counting as 0 from the first chunk that some term does not reach into (its padding is zero); byte b of the lengths gets one
// where OR & ~AND of the lengths is not zero.  Returns their number.
static uint32_t db_passes(const DbPlan &p, uint64_t n_terms, uint8_t *pos_pass /* 256 */, uint8_t *len_pass /* 2 */) {
    std::memset(pos_pass, 0, II2_DICT_BUILD_MAX_TERM);
    len_pass[0] = len_pass[1] = 0;
    if (n_terms == 0) return 0;
    uint32_t n = 0;
    const uint64_t lv = p.len_or & ~p.len_and;
    for (uint32_t b = 0; b < 2; b++)
        if ((lv >> (8u * b)) & 0xFFu) { len_pass[b] = 1; n++; }
    for (uint32_t c = 0; c < db_chunks(p.max_len); c++) {
        const uint64_t all = c < db_chunks(p.min_len) ? p.ch_and[c] : 0ull;
        const uint64_t v = p.ch_or[c] & ~all;
        for (uint32_t j = 0; j < 8; j++)
            if ((v >> (8u * (7u - j))) & 0xFFu) { pos_pass[8u * c + j] = 1; n++; }
    }
    return n;
}

__device__ __forceinline__ uint64_t db_wave_or(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
    return v;
}
__device__ __forceinline__ uint64_t db_wave_and(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v &= (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t db_wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ __forceinline__ uint32_t db_wave_min(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}

// bad |= 1: term_off does not start at 0, descends or leaves [0, term_off[n]]; bad |= 2: a term above II2_DICT_BUILD_MAX_TERM.
// Only a term whose offsets pass is read, so every byte read lies inside term_bytes[0 .. term_off[n]).  A workgroup strides over
// the terms: the lengths are reduced per lane, the chunks per wave into the wave's row of LDS, and at the end the workgroup's
// words go out with one atomic each (the grid is a few workgroups per CU: 125 000 waves adding to the same ten words took 7 ms).
__global__ __launch_bounds__(SB_THREADS) void k_db_plan(const uint8_t *__restrict__ bytes, const uint64_t *__restrict__ off, uint64_t n,
                                                        unsigned long long *ctl) {
    __shared__ unsigned long long s_or[SB_WAVES][DB_CHUNKS], s_and[SB_WAVES][DB_CHUNKS];
    __shared__ unsigned long long s_len[SB_WAVES][4];      // max, or, min, and of the wave's lengths
    __shared__ uint32_t s_bad[SB_WAVES];
    const uint32_t tid = threadIdx.x, w = tid >> 6, l = tid & 63u;
    if (l < DB_CHUNKS) { s_or[w][l] = 0ull; s_and[w][l] = ~0ull; }
    __syncthreads();
    uint32_t bad = 0, lmax = 0, lmin = 0xFFFFFFFFu, lor = 0, land = 0xFFFFFFFFu;
    const uint64_t end = off[n];
    for (uint64_t i0 = (uint64_t)blockIdx.x * SB_THREADS; i0 < n; i0 += (uint64_t)gridDim.x * SB_THREADS) {      // (uniform over the workgroup)
        const uint64_t i = i0 + tid;
        uint32_t len = 0;
        uint64_t b = 0;
        bool ok = false;
        if (i < n) {
            const uint64_t e = off[i + 1];
            b = off[i];
            if (e < b || e > end || (i == 0 && b != 0)) bad |= 1u;
            else if (e - b > II2_DICT_BUILD_MAX_TERM) bad |= 2u;
            else { ok = true; len = (uint32_t)(e - b); }
        }
        if (ok) { lmax = max(lmax, len); lmin = min(lmin, len); lor |= len; land &= len; }
        const uint32_t nc = ok ? db_chunks(len) : 0u, wave_nc = db_wave_max(nc);      // (wave_nc <= DB_CHUNKS: len <= the limit)
        for (uint32_t c = 0; c < wave_nc; c++) {
            const bool reach = c < nc;
            const uint64_t k = reach ? term_chunk(bytes + b, len, c) : 0ull;
            const uint64_t wor = db_wave_or(k), wand = db_wave_and(reach ? k : ~0ull);
            if (l == 0) { s_or[w][c] |= wor; s_and[w][c] &= wand; }
        }
    }
    lmax = db_wave_max(lmax); lmin = db_wave_min(lmin);
    lor = (uint32_t)db_wave_or(lor); land = (uint32_t)db_wave_and(0xFFFFFFFF00000000ull | land);
    bad = (uint32_t)db_wave_or(bad);
    if (l == 0) { s_len[w][0] = lmax; s_len[w][1] = lor; s_len[w][2] = lmin; s_len[w][3] = 0xFFFFFFFF00000000ull | land; s_bad[w] = bad; }
    __syncthreads();
    if (tid < DB_CHUNKS) {
        unsigned long long o = 0ull, a = ~0ull;
        for (uint32_t k = 0; k < SB_WAVES; k++) { o |= s_or[k][tid]; a &= s_and[k][tid]; }
        if (o) atomicOr(&ctl[DB_CTL_OR + tid], o);
        if (a != ~0ull) atomicAnd(&ctl[DB_CTL_AND + tid], a);
    } else if (tid == 64) {
        unsigned long long mx = 0ull, o = 0ull, mn = ~0ull, a = ~0ull;
        uint32_t bd = 0;
        for (uint32_t k = 0; k < SB_WAVES; k++) { mx = max(mx, s_len[k][0]); o |= s_len[k][1]; mn = min(mn, s_len[k][2]); a &= s_len[k][3]; bd |= s_bad[k]; }
        if (bd) atomicOr(&ctl[DB_CTL_BAD], (unsigned long long)bd);
        if (mn != 0xFFFFFFFFull) {      // some term of this workgroup passed
            atomicMax(&ctl[DB_CTL_MAX_LEN], mx);
            atomicMin(&ctl[DB_CTL_MIN_LEN], mn);
            atomicOr(&ctl[DB_CTL_LEN_OR], o);
            atomicAnd(&ctl[DB_CTL_LEN_AND], a & 0xFFFFFFFFull);
        }
    }
}

// key[i] = the length (c == DB_LEN) or chunk c of term idx[i]; init: the order is still the input's, idx[i] = i is stored
__global__ __launch_bounds__(SB_THREADS) void k_db_gather(const uint8_t *__restrict__ bytes, const uint64_t *__restrict__ off, uint64_t n, uint32_t *idx,
                                                          uint64_t *__restrict__ key, uint32_t c, int init) {
    const uint64_t i = (uint64_t)blockIdx.x * SB_THREADS + threadIdx.x;
    if (i >= n) return;
    uint32_t t = (uint32_t)i;
    if (init) idx[i] = t; else t = idx[i];
    const uint64_t b = off[t], len = off[t + 1] - b;
    key[i] = c == DB_LEN ? len : term_chunk(bytes + b, len, c);
}

__global__ __launch_bounds__(SB_THREADS) void k_db_hist(const uint64_t *__restrict__ keys, uint64_t n, uint32_t n_tiles, uint32_t shift,
                                                        uint32_t *__restrict__ count) {
    __shared__ uint32_t wcnt[SB_WAVES][SB_DIGITS];
    const uint32_t tid = threadIdx.x, w = tid >> 6;
    for (uint32_t k = 0; k < SB_WAVES; k++) wcnt[k][tid] = 0;
    __syncthreads();
    const uint64_t tile0 = (uint64_t)blockIdx.x * SB_TILE;
#pragma unroll 4
    for (uint32_t j = 0; j < SB_ITEMS; j++) {
        const uint64_t i = tile0 + (uint64_t)j * SB_THREADS + tid;
        const bool valid = i < n;
        sb_hist_count(wcnt[w], sb_digit(valid ? keys[i] : 0ull, shift), valid);
    }
    __syncthreads();
    sb_hist_store(wcnt, n_tiles, count);
}

// k_sb_scatter with a payload: the keys are ranked from registers, the indices meet them in LDS
__global__ __launch_bounds__(SB_THREADS) void k_db_scatter(const uint64_t *__restrict__ in_key, const uint32_t *__restrict__ in_idx, uint64_t *__restrict__ out_key,
                                                           uint32_t *__restrict__ out_idx, uint64_t n, uint32_t n_tiles, uint32_t shift,
                                                           const uint32_t *__restrict__ base) {
    __shared__ uint64_t stage[SB_TILE];
    __shared__ uint32_t sidx[SB_TILE];
    __shared__ uint32_t wcnt[SB_WAVES][SB_DIGITS];
    __shared__ uint32_t goff[SB_DIGITS];
    __shared__ uint32_t wsum[SB_WAVES];
    const uint32_t tid = threadIdx.x, w = tid >> 6, l = tid & 63u;
    const uint64_t tile0 = (uint64_t)blockIdx.x * SB_TILE;
    const uint32_t nv = n - tile0 < SB_TILE ? (uint32_t)(n - tile0) : SB_TILE;      // pairs of this tile
    for (uint32_t k = 0; k < SB_WAVES; k++) wcnt[k][tid] = 0;
    uint64_t key[SB_ITEMS];
    uint32_t rank[SB_ITEMS];
#pragma unroll
    for (uint32_t j = 0; j < SB_ITEMS; j++) {
        const uint32_t loc = w * SB_WAVE_KEYS + j * 64u + l;
        key[j] = loc < nv ? in_key[tile0 + loc] : 0ull;
    }
    __syncthreads();
    const uint64_t lt = (1ull << l) - 1ull;
#pragma unroll
    for (uint32_t j = 0; j < SB_ITEMS; j++) rank[j] = sb_wave_rank(sb_digit(key[j], shift), w * SB_WAVE_KEYS + j * 64u + l < nv, wcnt[w], l, lt);
    __syncthreads();
    sb_tile_bases(wcnt, goff, wsum, base, n_tiles);
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < SB_ITEMS; j++) {
        const uint32_t loc = w * SB_WAVE_KEYS + j * 64u + l;
        if (loc < nv) {
            const uint32_t slot = sb_stage_slot(wcnt, w, sb_digit(key[j], shift), rank[j]);
            stage[slot] = key[j];
            sidx[slot] = in_idx[tile0 + loc];
        }
    }
    __syncthreads();
    for (uint32_t s = tid; s < nv; s += SB_THREADS) {
        const uint64_t k = stage[s];
        const uint32_t g = goff[sb_digit(k, shift)] + s;
        out_key[g] = k;
        out_idx[g] = sidx[s];
    }
}

// WRITE == false: cnt[tile] = heads in the tile, ctl[DB_CTL_BYTES] += their lengths.  WRITE == true: cnt holds the exclusive scan
// of those counts; term_id[idx[i]] = rank of the run that holds sorted position i (term_id may be NULL), and head r leaves its
// length in ulen[r], its source index in usrc[r] and its chunk-0 key in dkey[r].
template <bool WRITE>
__global__ __launch_bounds__(SB_THREADS) void k_db_heads(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ idx, const uint8_t *__restrict__ bytes,
                                                         const uint64_t *__restrict__ off, uint64_t n, uint32_t long_terms, uint32_t *cnt,
                                                         unsigned long long *ctl, uint32_t *__restrict__ term_id, uint32_t *__restrict__ ulen,
                                                         uint32_t *__restrict__ usrc, uint64_t *__restrict__ dkey) {
    __shared__ uint32_t wsum[SB_WAVES];
    const uint32_t tid = threadIdx.x, w = tid >> 6, l = tid & 63u;
    const uint64_t wave0 = (uint64_t)blockIdx.x * SB_TILE + (uint64_t)w * SB_WAVE_KEYS;
    uint32_t heads = 0;      // bit j: item j of this lane is a head
    uint32_t run = 0;        // heads of this wave so far (wave-uniform)
    uint64_t sum = 0;        // lengths of this lane's heads
#pragma unroll 2
    for (uint32_t j = 0; j < SB_ITEMS; j++) {
        const uint64_t i = wave0 + j * 64u + l;
        const bool valid = i < n;
        const uint64_t k = valid ? keys[i] : 0ull;
        const uint32_t t = valid ? idx[i] : 0u;
        uint64_t pk = (uint64_t)__shfl_up((unsigned long long)k, 1, 64);
        uint32_t pt = (uint32_t)__shfl_up((int)t, 1, 64);
        if (l == 0 && valid && i > 0) { pk = keys[i - 1]; pt = idx[i - 1]; }
        bool head = false;
        if (valid) {
            const uint64_t b = off[t], len = off[t + 1] - b;
            head = i == 0 || k != pk;
            if (!head) {
                const uint64_t pb = off[pt], plen = off[pt + 1] - pb;
                head = term_cmp(k, bytes + b, len, pk, bytes + pb, plen, long_terms != 0) != 0;
            }
            if (head) { heads |= 1u << j; sum += len; }
        }
        run += (uint32_t)__popcll(__ballot(head));
    }
    if (l == 0) wsum[w] = run;
    if (!WRITE) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += (uint64_t)__shfl_xor((unsigned long long)sum, o, 64);
        if (l == 0 && sum) atomicAdd(&ctl[DB_CTL_BYTES], (unsigned long long)sum);
    }
    __syncthreads();
    if (!WRITE) {
        if (tid == 0) {
            uint32_t t = 0;
            for (uint32_t k = 0; k < SB_WAVES; k++) t += wsum[k];
            cnt[blockIdx.x] = t;
        }
        return;
    }
    uint32_t at = cnt[blockIdx.x];      // heads in front of this wave
    for (uint32_t k = 0; k < SB_WAVES; k++)
        if (k < w) at += wsum[k];
    const uint64_t le = (2ull << l) - 1ull;      // this lane and the lanes below it
#pragma unroll 2
    for (uint32_t j = 0; j < SB_ITEMS; j++) {
        const uint64_t i = wave0 + j * 64u + l;
        const bool head = (heads >> j) & 1u;
        const uint64_t m = __ballot(head);
        if (i < n) {
            const uint32_t r = at + (uint32_t)__popcll(m & le) - 1u;      // (position 0 is a head: at least one head is at or before i)
            const uint32_t t = idx[i];
            if (term_id) term_id[t] = r;
            if (head) {
                ulen[r] = (uint32_t)(off[t + 1] - off[t]);
                usrc[r] = t;
                dkey[r] = keys[i];
            }
        }
        at += (uint32_t)__popcll(m);
    }
}

// thread r: the bytes of dictionary term r, copied from source term usrc[r]
__global__ __launch_bounds__(SB_THREADS) void k_db_bytes(const uint8_t *__restrict__ bytes, const uint64_t *__restrict__ off, const uint32_t *__restrict__ usrc,
                                                         const uint64_t *__restrict__ doff, uint64_t n_unique, uint8_t *__restrict__ out) {
    const uint64_t r = (uint64_t)blockIdx.x * SB_THREADS + threadIdx.x;
    if (r >= n_unique) return;
    const uint64_t o = doff[r], len = doff[r + 1] - o;
    const uint8_t *src = bytes + off[usrc[r]];
    for (uint64_t j = 0; j < len; j++) out[o + j] = src[j];
}

}  // namespace ii2

using namespace ii2;

namespace {
// term_off as the caller of a host array gives it: EINVAL / ERANGE as the header says, II2_OK when every term may be read
int check_host_offsets(const uint64_t *term_off, uint64_t n) {
    if (term_off[0] != 0) return II2_EINVAL;
    bool too_long = false;
    for (uint64_t i = 0; i < n; i++) {
        if (term_off[i + 1] < term_off[i]) return II2_EINVAL;
        too_long |= term_off[i + 1] - term_off[i] > II2_DICT_BUILD_MAX_TERM;
    }
    return too_long ? II2_ERANGE : II2_OK;
}

// the dictionary's arrays, allocated as ii2_dict_create allocates them (~ii2_dict frees them)
int dict_alloc(ii2_ctx *ctx, uint64_t n, uint64_t n_bytes, uint32_t long_terms, std::unique_ptr<ii2_dict> *out) {
    std::unique_ptr<ii2_dict> d(new (std::nothrow) ii2_dict());
    if (!d) return II2_ENOMEM;
    d->device = ctx->device;
    d->n = n;
    d->n_bytes = n_bytes;
    d->long_terms = long_terms;
    if (dm_malloc_retry((void **)&d->d_off, (n + 1) * sizeof(uint64_t)) != hipSuccess || dm_malloc_retry((void **)&d->d_key, (n + 1) * sizeof(uint64_t)) != hipSuccess ||
        dm_malloc_retry((void **)&d->d_bytes, n_bytes + 16) != hipSuccess)
        return fail(ctx, II2_ENOMEM, "ii2_dict_build: allocation failed");
    *out = std::move(d);
    return II2_OK;
}
}  // namespace

extern "C" {

int ii2_dict_build(ii2_ctx *ctx, uint64_t n_terms, const uint8_t *term_bytes, const uint64_t *term_off, int where, ii2_dict **out, uint32_t *term_id,
                   ii2_dict_build_stats *stats) {
    if (!ctx || !out || (where != II2_HOST && where != II2_DEVICE)) return fail(ctx, II2_EINVAL, "ii2_dict_build: bad argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *out = nullptr;
    if (n_terms >= (1ull << 31)) return fail(ctx, II2_ERANGE, "ii2_dict_build: 2^31 or more terms; split the input");
    if (n_terms && (!term_bytes || !term_off)) return fail(ctx, II2_EINVAL, "ii2_dict_build: term_bytes or term_off is NULL");
    hipStream_t st = ctx->stream;
    const uint64_t n = n_terms;
    std::unique_ptr<ii2_dict> dict;
    if (n == 0) {
        if (int rc = dict_alloc(ctx, 0, 0, 0, &dict)) return rc;
        HIP_TRY(ctx, hipMemsetAsync(dict->d_off, 0, sizeof(uint64_t), st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (stats) std::memset(stats, 0, sizeof *stats);
        *out = dict.release();
        return II2_OK;
    }
    uint64_t n_in_bytes = 0;
    if (where == II2_HOST) {
        const int rc = check_host_offsets(term_off, n);
        if (rc == II2_EINVAL) return fail(ctx, rc, "ii2_dict_build: term_off must start at 0 and be non-decreasing");
        if (rc) return fail(ctx, rc, "ii2_dict_build: a term is longer than II2_DICT_BUILD_MAX_TERM bytes");
        n_in_bytes = term_off[n];
    }
    const size_t n_tiles = (size_t)((n + SB_TILE - 1) / SB_TILE);
    const size_t kw = align_up((size_t)n + 1, 64);      // words of a key or index buffer (its halves stay 256-byte aligned)
    const size_t tmpb = scan_temp_bytes(std::max<size_t>(SB_DIGITS * n_tiles, (size_t)n + 1));
    const size_t sz_key = align_up(kw * sizeof(uint64_t)), sz_idx = align_up(kw * sizeof(uint32_t)), sz_count = align_up(SB_DIGITS * n_tiles * sizeof(uint32_t)),
                 sz_tcnt = align_up((n_tiles + 1) * sizeof(uint32_t)), sz_in_bytes = where == II2_HOST ? align_up((size_t)n_in_bytes + 16) : 0,
                 sz_in_off = where == II2_HOST ? align_up((size_t)(n + 1) * sizeof(uint64_t)) : 0;
    BuildBlock blk(st);
    if (dm_alloc(&blk.p, 2 * sz_key + 2 * sz_idx + sz_count + align_up(tmpb) + sz_tcnt + sz_in_bytes + sz_in_off) != hipSuccess)
        return fail(ctx, II2_ENOMEM, "ii2_dict_build: device allocation failed");
    uint8_t *at = (uint8_t *)blk.p;
    uint64_t *key_a = (uint64_t *)at; at += sz_key;
    uint64_t *key_b = (uint64_t *)at; at += sz_key;
    uint32_t *idx_a = (uint32_t *)at; at += sz_idx;
    uint32_t *idx_b = (uint32_t *)at; at += sz_idx;
    uint32_t *d_count = (uint32_t *)at; at += sz_count;
    void *d_tmp = at; at += align_up(tmpb);
    uint32_t *d_tcnt = (uint32_t *)at; at += sz_tcnt;
    const uint8_t *d_bytes = term_bytes;
    const uint64_t *d_off = term_off;
    if (where == II2_HOST) {
        uint8_t *s_bytes = at; at += sz_in_bytes;
        uint64_t *s_off = (uint64_t *)at;
        if (n_in_bytes) HIP_TRY(ctx, hipMemcpyAsync(s_bytes, term_bytes, n_in_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(s_off, term_off, (size_t)(n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        d_bytes = s_bytes;
        d_off = s_off;
    }
    const dim3 block(SB_THREADS), grid_terms((unsigned)((n + SB_THREADS - 1) / SB_THREADS)), grid_tiles((unsigned)n_tiles);

    // the plan: one kernel, one readback (wait 1)
    unsigned long long *d_ctl = (unsigned long long *)(ctx->d_mail + II2_MAIL_DICT_BUILD);
    uint64_t *h_ctl = ctx->h_mail + II2_MAIL_DICT_BUILD;
    HIP_TRY(ctx, hipMemsetAsync(d_ctl, 0, DB_CTL_ONES * sizeof(uint64_t), st));
    HIP_TRY(ctx, hipMemsetAsync(d_ctl + DB_CTL_ONES, 0xFF, (DB_CTL_WORDS - DB_CTL_ONES) * sizeof(uint64_t), st));
    const dim3 grid_plan(std::min<unsigned>(grid_terms.x, 8u * (unsigned)std::max(ctx->cu_count, 1)));
    hipLaunchKernelGGL(k_db_plan, grid_plan, block, 0, st, d_bytes, d_off, n, d_ctl);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(h_ctl, d_ctl, DB_CTL_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (h_ctl[DB_CTL_BAD] & 1u) return fail(ctx, II2_EINVAL, "ii2_dict_build: term_off must start at 0 and be non-decreasing");
    if (h_ctl[DB_CTL_BAD] & 2u) return fail(ctx, II2_ERANGE, "ii2_dict_build: a term is longer than II2_DICT_BUILD_MAX_TERM bytes");
    DbPlan plan;
    plan.min_len = h_ctl[DB_CTL_MIN_LEN]; plan.max_len = h_ctl[DB_CTL_MAX_LEN];
    plan.len_or = h_ctl[DB_CTL_LEN_OR]; plan.len_and = h_ctl[DB_CTL_LEN_AND];
    for (uint32_t c = 0; c < DB_CHUNKS; c++) { plan.ch_or[c] = h_ctl[DB_CTL_OR + c]; plan.ch_and[c] = h_ctl[DB_CTL_AND + c]; }
    uint8_t pos_pass[II2_DICT_BUILD_MAX_TERM], len_pass[2];
    const uint32_t n_passes = db_passes(plan, n, pos_pass, len_pass);

    // the sort: the length is the least significant key, then the chunks from the last to the first
    uint64_t *src_k = key_a, *dst_k = key_b;
    uint32_t *src_i = idx_a, *dst_i = idx_b;
    bool ordered = false;      // idx holds an order (else it is still to be set to the input's)
    auto gather = [&](uint32_t c) {
        hipLaunchKernelGGL(k_db_gather, grid_terms, block, 0, st, d_bytes, d_off, n, src_i, src_k, c, ordered ? 0 : 1);
        ordered = true;
        return hipGetLastError();
    };
    auto pass = [&](uint32_t shift) {
        hipLaunchKernelGGL(k_db_hist, grid_tiles, block, 0, st, (const uint64_t *)src_k, n, (uint32_t)n_tiles, shift, d_count);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = scan_excl_u32(d_tmp, tmpb, d_count, d_count, SB_DIGITS * n_tiles, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_db_scatter, grid_tiles, block, 0, st, (const uint64_t *)src_k, (const uint32_t *)src_i, dst_k, dst_i, n, (uint32_t)n_tiles, shift,
                           (const uint32_t *)d_count);
        std::swap(src_k, dst_k);
        std::swap(src_i, dst_i);
        return hipGetLastError();
    };
    if (len_pass[0] || len_pass[1]) {
        HIP_TRY(ctx, gather(DB_LEN));
        for (uint32_t b = 0; b < 2; b++)
            if (len_pass[b]) HIP_TRY(ctx, pass(8u * b));
    }
    for (uint32_t c = std::max(db_chunks(plan.max_len), 1u); c-- > 0;) {
        bool any = c == 0;      // chunk 0 is gathered in any case: the final keys are the dictionary's
        for (uint32_t j = 0; j < 8; j++) any |= pos_pass[8u * c + j] != 0;
        if (!any) continue;
        HIP_TRY(ctx, gather(c));
        for (uint32_t j = 8; j-- > 0;)
            if (pos_pass[8u * c + j]) HIP_TRY(ctx, pass(8u * (7u - j)));
    }

    // equal terms are neighbours now: count the heads and their bytes (wait 2), then number the runs
    const uint32_t long_terms = plan.max_len > 8 ? 1u : 0u;
    uint32_t *d_ulen = (uint32_t *)dst_k, *d_usrc = (uint32_t *)dst_k + kw;      // the free key buffer: [n + 1] lengths, [n] source indices
    HIP_TRY(ctx, hipMemsetAsync(d_tcnt + n_tiles, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_db_heads<false>, grid_tiles, block, 0, st, (const uint64_t *)src_k, (const uint32_t *)src_i, d_bytes, d_off, n, long_terms, d_tcnt, d_ctl,
                       (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint64_t *)nullptr);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, scan_excl_u32(d_tmp, tmpb, d_tcnt, d_tcnt, n_tiles + 1, st));
    uint32_t n_unique32 = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&h_ctl[DB_CTL_BYTES], d_ctl + DB_CTL_BYTES, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(&h_ctl[DB_CTL_BAD], d_tcnt + n_tiles, sizeof(uint32_t), hipMemcpyDeviceToHost, st));      // (the word is free again)
    HIP_TRY(ctx, hipStreamSynchronize(st));
    n_unique32 = (uint32_t)h_ctl[DB_CTL_BAD];
    const uint64_t n_unique = n_unique32, n_bytes = h_ctl[DB_CTL_BYTES];
    if (int rc = dict_alloc(ctx, n_unique, n_bytes, long_terms, &dict)) return rc;
    uint32_t *d_term_id = term_id;
    if (term_id && where == II2_HOST) d_term_id = dst_i;      // staged in the free index buffer
    hipLaunchKernelGGL(k_db_heads<true>, grid_tiles, block, 0, st, (const uint64_t *)src_k, (const uint32_t *)src_i, d_bytes, d_off, n, long_terms, d_tcnt, d_ctl,
                       d_term_id, d_ulen, d_usrc, dict->d_key);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemsetAsync(d_ulen + n_unique, 0, sizeof(uint32_t), st));
    HIP_TRY(ctx, scan_excl_u32_to_u64(d_tmp, tmpb, d_ulen, dict->d_off, (size_t)n_unique + 1, st));
    hipLaunchKernelGGL(k_db_bytes, dim3((unsigned)((n_unique + SB_THREADS - 1) / SB_THREADS)), block, 0, st, d_bytes, d_off, (const uint32_t *)d_usrc,
                       (const uint64_t *)dict->d_off, n_unique, dict->d_bytes);
    HIP_TRY(ctx, hipGetLastError());
    if (term_id && where == II2_HOST) HIP_TRY(ctx, hipMemcpyAsync(term_id, d_term_id, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));      // wait 3: the end
    *out = dict.release();
    if (stats) {
        stats->n_terms = n;
        stats->n_unique = n_unique;
        stats->n_bytes = n_bytes;
        stats->min_len = (uint32_t)plan.min_len;
        stats->max_len = (uint32_t)plan.max_len;
        stats->n_passes = n_passes;
        stats->pad = 0;
    }
    return II2_OK;
}

int ii2_dict_info(const ii2_dict *dict, uint64_t *n_terms, uint64_t *n_bytes) {
    if (!dict) return II2_EINVAL;
    if (n_terms) *n_terms = dict->n;
    if (n_bytes) *n_bytes = dict->n_bytes;
    return II2_OK;
}

int ii2_dict_export(ii2_ctx *ctx, const ii2_dict *dict, uint8_t *term_bytes, uint64_t *term_off) {
    if (!ctx || !dict || dict->device != ctx->device) return fail(ctx, II2_EINVAL, "ii2_dict_export: bad argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (term_bytes && dict->n_bytes) HIP_TRY(ctx, hipMemcpyAsync(term_bytes, dict->d_bytes, dict->n_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (term_off) HIP_TRY(ctx, hipMemcpyAsync(term_off, dict->d_off, (dict->n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return II2_OK;
}

// host only: chunk c of one term, by term_chunk
int ii2_term_chunk(const uint8_t *term, uint64_t len, uint32_t c, uint64_t *key) {
    if (!key || (len && !term)) return II2_EINVAL;
    *key = term_chunk(term, len, c);
    return II2_OK;
}

// host only: the reduction of k_db_plan as a loop, then db_passes - the function the driver turns the kernel's words into passes with
int ii2_dict_build_plan(const uint8_t *term_bytes, const uint64_t *term_off, uint64_t n_terms, uint8_t *pos_pass, uint8_t *len_pass, uint32_t *n_passes,
                        uint32_t *min_len, uint32_t *max_len) {
    if (!pos_pass || !len_pass || !n_passes || !min_len || !max_len) return II2_EINVAL;
    if (n_terms >= (1ull << 31)) return II2_ERANGE;
    if (n_terms && (!term_bytes || !term_off)) return II2_EINVAL;
    DbPlan p;
    std::memset(&p, 0, sizeof p);
    if (n_terms) {
        if (int rc = check_host_offsets(term_off, n_terms)) return rc;
        p.min_len = p.len_and = ~0ull;
        std::memset(p.ch_and, 0xFF, sizeof p.ch_and);
    }
    for (uint64_t i = 0; i < n_terms; i++) {
        const uint64_t b = term_off[i], len = term_off[i + 1] - b;
        p.min_len = std::min(p.min_len, len);
        p.max_len = std::max(p.max_len, len);
        p.len_or |= len;
        p.len_and &= len;
        for (uint32_t c = 0; c < db_chunks(len); c++) {
            const uint64_t k = term_chunk(term_bytes + b, len, c);
            p.ch_or[c] |= k;
            p.ch_and[c] &= k;
        }
    }
    *n_passes = db_passes(p, n_terms, pos_pass, len_pass);
    *min_len = (uint32_t)p.min_len;
    *max_len = (uint32_t)p.max_len;
    return II2_OK;
}

}  // extern "C"
