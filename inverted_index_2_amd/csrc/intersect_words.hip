// intersect_words.hip — AND of two lists that BOTH have a dense form (a bitmap over the list's docs, made once and cached with the
// segment's store: setop.cpp dense_form_get), gfx950, wave64, no MFMA.  Semantics as intersect_and2.hip: ascending ids present in
// both lists, minus the tombstoned ones.
//
// The result's bitmap is wa[i] & wb[i] & ~tomb[i]: no skip table, no payload, no varint, no LDS bitmap, no per-posting test - and
// no load that depends on another one.  The window both forms cover is cut into runs of AW_W words, one per workgroup; a wave owns
// AW_K chunks of 256 consecutive words, 16 bytes a lane of each array, all requested at once.  The ids a workgroup will write are
// the set bits of its words: counted (popcount) and published to the look-back (lookback.h) before a single bit is extracted.
//
// Extraction.  A lane walks ITS 128 bits of a chunk - four words, one after the other, in one loop that ends with the lane's
// last bit: the wave runs as long as its fullest lane of 128 bits (32 steps for 21 set bits at one doc in six: two thirds of the
// lanes' steps place an id), not as long as the fullest of 64 words four times over (44).  Every bit becomes a 16-bit offset from
// the chunk's first doc at its place in the chunk's stage; a stage goes out 16 bytes a lane, coalesced, at any 4-byte alignment.
// A stage holds AW_STAGE ids whatever the density: a chunk with more ids (up to 8192: every bit set) takes several rounds, the
// lanes carry their position across them.  Every chunk has a stage of its own: the first round of all of them is staged while the
// look-back record travels, and the stores then go out in one run (one stage for both chunks, the second one staged between the
// two runs of stores: 22.0 us against 20.4 on the 100M-doc pair of DESIGN.md 4.1a').
//
// Two things about the stores are template parameters (options intersect.and2_words_order / intersect.and2_words_store):
//   WT     (the default) the id stores are write-through (sc1): the bytes leave the XCD's L2 as they are stored, none stay dirty
//          for the kernel's end to write back - 19.0 us against 21.7 with plain stores.  A partial 128-byte line then goes to
//          the fabric as it is, so the 16-byte stores go to 16-byte-aligned addresses: a head of up to three single ids, the
//          aligned body, a tail of single ids.  The stores go through a buffer resource that starts at the workgroup's first
//          id and ends with its last one or with the capacity, whichever comes first.
//   EARLY  (measurements: it loses, 20.1 us with WT and 23.2 without) only chunk 0 is staged while the record travels; its
//          stores leave as soon as the workgroup's offset is known and chunk 1 is staged behind them (stage c0 / flush c0 /
//          stage c1 / flush c1).
#include "dv1_device.h"
#include "internal.h"
#include "lookback.h"

namespace ii2 {

constexpr uint32_t AW_K = 2;                                  // chunks a wave owns: 16-byte loads a lane of each array
constexpr uint32_t AW_CHUNK = 256;                            // words of a chunk (4 per lane): 8192 docs, offsets of 13 bits
constexpr uint32_t AW_WAVE = AW_K * AW_CHUNK;                 // words of a wave ...
constexpr uint32_t AW_W = 4u * AW_WAVE;                       // ... and of a workgroup
constexpr uint32_t AW_STAGE = 1536;                           // ids a chunk stages per round (a chunk at one doc in six has 1365 +- 34)
static_assert(AW_STAGE % 256u == 0u, "a round is flushed four ids a lane");

__device__ __forceinline__ uint32_t aw_uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }

struct AwLane {                 // a lane's bits of one chunk that are not staged yet, and where the next one goes
    uint32_t x, w1, w2, w3;     // the word being walked, then the words behind it
    uint32_t base;              // bit number, within the chunk, of x's bit 0
    uint32_t q, qend;           // place among the chunk's ids of my next bit / behind my last one
};

// My bits whose places lie in [rb, rb + AW_STAGE), as 16-bit offsets at st[place - rb].  A step either places the lowest bit of x
// or - x used up - moves on to the next word; such a step writes a value nobody reads over the place of the lane's next id, which
// is written again when that id comes (same lane, program order).  q < qend says that a bit is left: the walk never runs dry
__device__ __forceinline__ void aw_stage(uint16_t *st, AwLane &L, uint32_t rb) {
    const uint32_t lim = rb + AW_STAGE;
    const uint32_t stop = L.qend < lim ? L.qend : lim;
    while (L.q < stop) {
        const bool e = L.x == 0u;
        const uint32_t b = (uint32_t)__builtin_ctz(e ? 1u : L.x);      // lowest set bit (x = 0: any value will do)
        st[L.q - rb] = (uint16_t)(L.base + b);
        L.q += e ? 0u : 1u;
        L.x = e ? L.w1 : (L.x & (L.x - 1u));
        L.w1 = e ? L.w2 : L.w1;
        L.w2 = e ? L.w3 : L.w2;
        L.base += e ? 32u : 0u;
    }
}

// n staged ids out to out[pos ...): 16 bytes a lane (wave-private LDS: program order is enough).  Nothing at or beyond out_cap
__device__ __forceinline__ void aw_flush(const DenseParams &p, const uint16_t *st, uint32_t n, uint32_t doc0, unsigned long long pos) {
    const uint32_t l = (uint32_t)lane_id();
    const bool fits = pos + n <= p.out_cap;
    for (uint32_t c = 4u * l; c < n; c += 256u) {
        const uint2 pk = *reinterpret_cast<const uint2 *>(&st[c]);
        const uint4 ids = make_uint4(doc0 + (pk.x & 0xFFFFu), doc0 + (pk.x >> 16), doc0 + (pk.y & 0xFFFFu), doc0 + (pk.y >> 16));
        if (c + 4u <= n && fits) {
            uint32_t *dst = p.out + pos + c;
            __builtin_memcpy(dst, &ids, 16);                    // one 16-byte store, any 4-byte alignment
        } else {
            const uint32_t vv[4] = {ids.x, ids.y, ids.z, ids.w};
            for (uint32_t k = 0; k < 4u; k++)
                if (c + k < n && pos + c + k < p.out_cap) p.out[pos + c + k] = vv[k];
        }
    }
}

// the same, write-through and aligned (WT above).  rs covers out[wg_off, wg_off + lim): rel = the round's first place in it,
// mis = the ids by which out + wg_off lies behind a 16-byte boundary.  Stage reads at any 2-byte alignment.  (A head of up to 31
// ids, so that a wave instruction's 1 KB starts on a 128-byte line: 18.9 us against 19.0, not kept)
__device__ __forceinline__ void aw_store1(uint32_t v, __amdgpu_buffer_rsrc_t rs, uint32_t place) {
    __builtin_amdgcn_raw_buffer_store_b32(v, rs, (int)(4u * place), 0, 16);              // (aux 16 = sc1)
}
__device__ __forceinline__ void aw_flush_wt(const uint16_t *st, uint32_t n, uint32_t doc0, __amdgpu_buffer_rsrc_t rs, uint32_t rel, uint32_t lim, uint32_t mis) {
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const uint32_t l = (uint32_t)lane_id();
    if (rel + n > lim) {                                            // the capacity edge: id by id
        for (uint32_t c = l; c < n; c += 64u)
            if (rel + c < lim) aw_store1(doc0 + st[c], rs, rel + c);
        return;
    }
    const uint32_t h0 = (0u - (mis + rel)) & 3u;
    const uint32_t h = h0 < n ? h0 : n;                             // head: up to the first aligned place
    if (l < h) aw_store1(doc0 + st[l], rs, rel + l);
    const uint32_t nb = (n - h) & ~3u;                              // body: 16 bytes a lane
    for (uint32_t c = 4u * l; c < nb; c += 256u) {
        uint16_t o[4];
        __builtin_memcpy(o, &st[h + c], 8);
        const v4u ids = {doc0 + o[0], doc0 + o[1], doc0 + o[2], doc0 + o[3]};
        __builtin_amdgcn_raw_buffer_store_b128(ids, rs, (int)(4u * (rel + h + c)), 0, 16);
    }
    const uint32_t t0 = h + nb;                                     // tail: up to three ids
    if (t0 + l < n) aw_store1(doc0 + st[t0 + l], rs, rel + t0 + l);
}

template <bool EARLY, bool WT>
__global__ __launch_bounds__(256, 6) void k_and2_words(DenseParams p) {
    __shared__ __align__(16) uint16_t stage[4][AW_K][AW_STAGE + 8];      // (+ the flush's read-ahead)
    __shared__ uint32_t wcnt[4];
    __shared__ unsigned long long wg_off;
    __shared__ uint32_t wg_err;
    const uint32_t l = (uint32_t)lane_id();
    const uint32_t wv = aw_uni(threadIdx.x >> 6);
    const uint32_t g = blockIdx.x;
    if (p.w_n == 0u) {                                       // no common doc (one workgroup): the count, nothing else
        if (threadIdx.x == 0) *p.d_count = 0ull;
        return;
    }
    unsigned long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tprev = 0;
    const bool stamps = p.debug != nullptr;
#define II2_STAMP(i)                                                    \
    if (stamps) {                                                       \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");              \
        const unsigned long long tn_ = __builtin_amdgcn_s_memtime();    \
        tacc[i] += tn_ - tprev;                                         \
        tprev = tn_;                                                    \
    }
    if (stamps) tprev = __builtin_amdgcn_s_memtime();
    if (threadIdx.x == 0) wg_err = 0u;

    // ---- one go: my words of both forms and of the tombstone bitmap.  i0 = my first word's place in the window; the forms'
    // places of the window's first word differ (at most one of them is a multiple of four words: 16-byte loads at 4-byte
    // alignment).  Every lane loads - from a place clamped into the window or the bitmap, so up to three words past the last
    // one: a form carries 16 bytes of padding (setop.cpp dense_form_get), a tombstone bitmap TOMB_PAD_WORDS words (api.cpp
    // ii2_tomb_create) - and what lies outside is zeroed once it has landed
    static_assert(TOMB_PAD_WORDS >= 3u, "a 16-byte load from a tombstone bitmap's last word stays inside its allocation");
    const uint32_t wi = g * AW_W + wv * AW_WAVE + 4u * l;
    const uint32_t oa = p.w_lo - (p.a_origin >> 5), ob = p.w_lo - (p.b_origin >> 5);
    const bool tombs = p.tomb != nullptr && p.tomb_nwords != 0u;
    uint4 A[AW_K], B[AW_K], T[AW_K];
#pragma unroll
    for (uint32_t c = 0; c < AW_K; c++) {
        const uint32_t i0 = wi + c * AW_CHUNK;
        const uint32_t ic = i0 < p.w_n ? i0 : p.w_n - 1u;
        // (32-bit byte offsets from the uniform bases: a form has <= 2^27 words)
        __builtin_memcpy(&A[c], reinterpret_cast<const uint8_t *>(p.a_bits) + 4u * (oa + ic), 16);
        __builtin_memcpy(&B[c], reinterpret_cast<const uint8_t *>(p.b_bits) + 4u * (ob + ic), 16);
    }
    if (tombs) {
#pragma unroll
        for (uint32_t c = 0; c < AW_K; c++) {
            const uint32_t ti = p.w_lo + wi + c * AW_CHUNK;
            const uint32_t tc = ti < p.tomb_nwords ? ti : p.tomb_nwords - 1u;
            __builtin_memcpy(&T[c], reinterpret_cast<const uint8_t *>(p.tomb) + 4u * tc, 16);
        }
    }
    II2_STAMP(0)              // requests
    AwLane L[AW_K];
    uint32_t pc[AW_K];
#pragma unroll
    for (uint32_t c = 0; c < AW_K; c++) {
        const uint32_t i0 = wi + c * AW_CHUNK;
        uint32_t r[4] = {A[c].x & B[c].x, A[c].y & B[c].y, A[c].z & B[c].z, A[c].w & B[c].w};
        if (tombs) {
            const uint32_t ti = p.w_lo + i0;
            const uint32_t t[4] = {T[c].x, T[c].y, T[c].z, T[c].w};
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) r[j] &= ~(ti + j < p.tomb_nwords ? t[j] : 0u);
        }
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) r[j] = i0 + j < p.w_n ? r[j] : 0u;
        L[c].x = r[0]; L[c].w1 = r[1]; L[c].w2 = r[2]; L[c].w3 = r[3];
        L[c].base = 128u * l;
        pc[c] = (uint32_t)(__popc(r[0]) + __popc(r[1]) + __popc(r[2]) + __popc(r[3]));
    }
    // ---- count first: the ids of the wave's chunks, of the workgroup - published before any bit is extracted
    uint32_t ctot[AW_K], count = 0;
#pragma unroll
    for (uint32_t c = 0; c < AW_K; c++) {
        const uint32_t incl = wave_incl_scan(pc[c]);
        ctot[c] = wave_bcast(incl, 63);
        L[c].qend = incl;
        L[c].q = incl - pc[c];
        count += ctot[c];
    }
    if (l == 0) wcnt[wv] = count;
    lds_barrier();
    const uint32_t c0 = wcnt[0], c1 = wcnt[1], c2 = wcnt[2], c3 = wcnt[3];
    const uint32_t total = c0 + c1 + c2 + c3;
    const uint32_t before = wv == 0u ? 0u : wv == 1u ? c0 : wv == 2u ? c0 + c1 : c0 + c1 + c2;
    if (threadIdx.x == 0) lb_publish(p.lb, g, total);
    II2_STAMP(1)              // landing, count, barrier, publish
    if (wv == 1u && lb_is_leader(g, gridDim.x)) {            // the group's ids, as soon as its other members have published theirs
        if (!lb_group_publish(p.lb, g, total) && l == 0) { wg_err = 1u; lb_fail(p.lb); }
    }
    // ---- while the record travels: the first round of every chunk (EARLY: of chunk 0) into its stage
#pragma unroll
    for (uint32_t c = 0; c < (EARLY ? 1u : AW_K); c++) aw_stage(stage[wv][c], L[c], 0u);
    II2_STAMP(2)              // stage, first rounds
    // ---- the ids of all workgroups before mine (wave 0)
    if (wv == 0u) {
        unsigned long long pre = 0ull;
        const bool ok = lb_prefix(p.lb, g, gridDim.x, total, &pre);
        bool late = false;                  // (tests: a give-up after the last workgroup has stored the count - lookback.h)
        if (p.lb.spin == LB_SPIN_LATE && ok && total != 0u && lb_late_pick(g, gridDim.x)) late = lb_late_wait(p.lb);
        if (l == 0) {
            wg_off = ok ? pre : 0ull;
            if (!ok || late) { wg_err = 1u; lb_fail(p.lb); }
        }
    }
    II2_STAMP(3)              // look-back
    lds_barrier();
    const bool err = wg_err != 0u;
    if (g == gridDim.x - 1u && threadIdx.x == 0) {          // the last workgroup: the total, or all ones when some workgroup gave up
        const bool anyerr = err || lb_failed(p.lb);
        *p.d_count = anyerr ? ~0ull : wg_off + total;
        if (p.lb.spin == LB_SPIN_LATE) lb_late_done(p.lb);
    }
    // ---- out: chunk by chunk, round by round (a round that is staged already: staging it again places nothing).  EARLY: chunk
    // 1's first round is staged here, behind chunk 0's stores
    if (!err && count != 0u) {
        unsigned long long pos = wg_off + before;
        const uint32_t doc_wave = 32u * (p.w_lo + g * AW_W + wv * AW_WAVE);
        // (WT) the workgroup's ids as a buffer: from its first id to its last one or to the capacity
        const unsigned long long wgo = wg_off;
        const uint32_t off_lo = aw_uni((uint32_t)wgo), off_hi = aw_uni((uint32_t)(wgo >> 32));
        const unsigned long long base = ((unsigned long long)off_hi << 32) | off_lo;
        const unsigned long long room = p.out_cap > base ? p.out_cap - base : 0ull;
        const uint32_t lim = room < total ? (uint32_t)room : total;
        const uint32_t mis = (uint32_t)((uintptr_t)(p.out + base) >> 2) & 3u;
        __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(p.out + base, 0, (int)(4u * lim), 0x00020000);
        uint32_t rel = before;
#pragma unroll
        for (uint32_t c = 0; c < AW_K; c++) {
            uint16_t *st = stage[wv][c];
            for (uint32_t rb = 0; rb < ctot[c]; rb += AW_STAGE) {
                aw_stage(st, L[c], rb);
                __builtin_amdgcn_wave_barrier();
                if (c == 1u && rb == 0u) { II2_STAMP(5) }      // stage c1 (not EARLY: staged already)
                const uint32_t n = ctot[c] - rb < AW_STAGE ? ctot[c] - rb : AW_STAGE;
                if (WT) aw_flush_wt(st, n, doc_wave + 32u * AW_CHUNK * c, rs, rel + rb, lim, mis);
                else aw_flush(p, st, n, doc_wave + 32u * AW_CHUNK * c, pos + rb);
                __builtin_amdgcn_wave_barrier();
            }
            pos += ctot[c];
            rel += ctot[c];
            if (c == 0u) { II2_STAMP(4) } else { II2_STAMP(6) }   // flush c0 / flush c1 (and the staging of rounds behind the first)
        }
    }
    if (stamps && l == 0)
        for (int i = 0; i < 8; i++) atomicAdd(&p.debug[(uint64_t)(blockIdx.x % 2048u) * 8u + i], tacc[i]);
#undef II2_STAMP
}

uint32_t and2_words_plan(DenseParams &p) {
    const uint32_t wa = p.a_origin >> 5, wb = p.b_origin >> 5;
    const uint32_t lo = wa > wb ? wa : wb;
    const uint32_t ea = wa + p.a_nwords, eb = wb + p.b_nwords;             // (<= 2^27 + 2^27: no wrap)
    const uint32_t hi = ea < eb ? ea : eb;
    p.w_lo = lo;
    p.w_n = hi > lo ? hi - lo : 0u;
    return p.w_n ? (p.w_n + AW_W - 1u) / AW_W : 1u;
}

hipError_t launch_and2_words(const DenseParams &p, hipStream_t s) {
    const uint32_t grid = p.w_n ? (p.w_n + AW_W - 1u) / AW_W : 1u;
    const dim3 gd(grid), bd(256);
#define II2_AW(E, W) hipLaunchKernelGGL((k_and2_words<E, W>), gd, bd, 0, s, p)
    if (p.words_early) { if (p.words_store) II2_AW(true, true); else II2_AW(true, false); }
    else { if (p.words_store) II2_AW(false, true); else II2_AW(false, false); }
#undef II2_AW
    return hipGetLastError();
}

}  // namespace ii2
