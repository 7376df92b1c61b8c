// intersect_and2.hip — AND of TWO lists that are dense together (BASELINE configs[1]: the 2-term query over a 100M-doc
// index), gfx950, wave64, no MFMA.  Semantics: SURVEY §8 a14 (ascending ids present in both lists, minus the
// tombstoned ones); reading without tombstones = /root/reference shard.go:72-75.
//
// intersect_dense.hip treats its 2..4 lists alike: every list is marked into a wave-private LDS bitmap, the bitmaps are
// ANDed, the result words go to HBM and a second kernel digs the set bits out of them one by one (a loop that runs as
// long as the fullest of 64 words has bits).  For two lists that is more work than the problem holds:
//   * only the LONGER list (A) is marked;
//   * the SHORTER list (B) paces the rounds — a wave owns 16 of its blocks, a row of four lanes per block, 64 payload
//     bytes per lane — and every B posting is TESTED against A's bitmap where it sits in the lane's registers: a
//     running add per gap byte, one LDS read, one bit-field extract.  The answers are one bit per B posting (H, 64 bits
//     per lane, bit j = posting 64 * row-lane + j of the row's block: the posting before the lane's bytes, then its
//     bytes 0..62);
//   * the result ids ARE B postings: the second kernel re-walks the lane's bytes with H as the write mask — no bitmap
//     round trip through HBM (4 MB of H instead of 2 x 13 MB of result words), no per-bit extraction loop, and every
//     lane has the same 64 steps (no fullest-word imbalance).
// Exact for any input the general kernel accepts: A's blocks go through the same marking as intersect_dense.hip (multi-
// byte gaps, wide groups, short blocks), rounds wider than the LDS window are split, B blocks with multi-byte gaps are
// decoded by the whole wave and answer by posting index through a small LDS scratch.
#include <algorithm>

#include "dv1_device.h"
#include "internal.h"
#include "lookback.h"

namespace ii2 {

constexpr uint32_t A2_ROWS = 16;                              // blocks per pass: one per row of four lanes, 64 payload bytes per lane
constexpr uint32_t A2_GU = 512;                               // guard bits below and above a window (a lane of narrow groups spans < 512 docs)
constexpr uint32_t A2_CAPW = DENSE_CAPW;                      // docs a window covers (multiple of 32)
constexpr uint32_t A2_NW = ((A2_CAPW + 2 * A2_GU) / 32 + 2 + 3) & ~3u;    // words of the LDS bitmap (a multiple of 4: 16-byte clears)
constexpr uint32_t A2_HS = A2_ROWS * 8;                       // hard rows of B: 256 answer bits per row
constexpr uint32_t A2_WAVE_LDS = A2_NW + A2_HS;
constexpr uint32_t A2_STAGE = A2_ROWS * 256 + 8;              // u16 ids a wave stages (every posting of 16 full blocks + the flush's read-ahead)

__device__ __forceinline__ uint32_t a2_uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }

// first index i in [0, n) with skip[i].first_doc > x, searched 64 ways per round by the whole wave
__device__ __forceinline__ uint32_t a2_skip_upper_bound(const ii2_skip *__restrict__ skip, uint32_t n, uint32_t x) {
    const uint32_t l = (uint32_t)lane_id();
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t sp = hi - lo;
        const uint32_t st = (sp + 63u) >> 6;
        const uint32_t pos = lo + l * st;
        const bool in = pos < hi;
        const uint32_t f = in ? skip[pos].first_doc : 0u;
        const uint32_t cnt = (uint32_t)__popcll(__ballot(in && f <= x));     // probes are ascending: the matches are a prefix
        const uint32_t nin = (uint32_t)__popcll(__ballot(in));
        if (st == 1u) return cnt < nin ? lo + cnt : hi;
        const uint32_t nlo = cnt ? lo + (cnt - 1u) * st + 1u : lo;
        hi = cnt < nin ? lo + cnt * st : hi;
        lo = nlo;
    }
    return lo;
}

struct A2Bytes { uint4 g[4]; };

// my row's skip entry and the next one, for the blocks [at, at + 16) of a list (indices clamped onto the readable entry nblk)
__device__ __forceinline__ uint4 a2_ent_load(const ListView &L, uint32_t at, uint32_t row) {
    const uint32_t i0 = at + row < L.nblk ? at + row : L.nblk;
    const uint32_t i1 = i0 < L.nblk ? i0 + 1u : L.nblk;
    const ii2_skip e0 = L.skip[i0], e1 = L.skip[i1];
    return make_uint4(e0.first_doc, e0.byte_off, e1.first_doc, e1.byte_off);
}

// 64 payload bytes of my row's block [q0, q1): lane rl of the row takes bytes [64 rl, 64 rl + 64) (zero past the block's end at 16-byte grain)
__device__ __forceinline__ A2Bytes a2_fetch(const uint8_t *payload, bool rv, uint32_t q0, uint32_t q1, uint32_t rl) {
    const uint32_t len = rv ? q1 - q0 : 0u;
    A2Bytes B;
    const uint8_t *src = payload + q0 + 64u * rl;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        B.g[k] = make_uint4(0, 0, 0, 0);
        if (len > 64u * rl + 16u * k) __builtin_memcpy(&B.g[k], src + 16u * k, 16);   // segments carry 16 bytes of padding
    }
    return B;
}

// The lane's 64 bytes as sixteen words.  A FULL block of one-byte gaps has 255 payload bytes: the row's last lane holds one byte
// that is not its own (zeroed here).  Every other block of a valid row — a list's short last block, a block with a multi-byte
// gap — is `hard`: it goes through the general wave decoder, which takes any block.  Returns the ballot of the hard rows' lanes.
__device__ __forceinline__ unsigned long long a2_prep(const A2Bytes &B, bool rv, uint32_t len, uint32_t rl, uint32_t (&ww)[16]) {
    ww[0] = B.g[0].x; ww[1] = B.g[0].y; ww[2] = B.g[0].z; ww[3] = B.g[0].w;
    ww[4] = B.g[1].x; ww[5] = B.g[1].y; ww[6] = B.g[1].z; ww[7] = B.g[1].w;
    ww[8] = B.g[2].x; ww[9] = B.g[2].y; ww[10] = B.g[2].z; ww[11] = B.g[2].w;
    ww[12] = B.g[3].x; ww[13] = B.g[3].y; ww[14] = B.g[3].z;
    ww[15] = rl == 3u ? (B.g[3].w & 0x00FFFFFFu) : B.g[3].w;
    uint32_t any = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16u; k++) any |= ww[k];
    const bool hard = rv && (len != 255u || (any & 0x80808080u) != 0u);
    return __ballot(hard);
}

// id of the posting right before my bytes: the block's first doc + the gap sums of the row's lanes before me (rows of
// one-byte gaps only; `live` = my row is one).  *wide_or = OR of my sixteen group sums (a bit above bit 4 = some group of four
// postings spans 32 docs or more).
__device__ __forceinline__ uint32_t a2_group_sum(uint32_t x) {      // sum of a word's four bytes; opaque, so that the compiler recomputes it where it
    uint32_t g;                                                       // is needed instead of keeping sixteen of them (or their prefix sums) in registers
    asm volatile("v_sad_u8 %0, %1, 0, 0" : "=v"(g) : "v"(x));
    return g;
}
__device__ __forceinline__ uint32_t a2_lane_base(const uint32_t (&ww)[16], bool live, uint32_t f, uint32_t rl, uint32_t *wide_or) {
    uint32_t acc = 0, wide = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16u; k += 2u) {                             // (two groups per step: three-input or / add)
        const uint32_t g0 = a2_group_sum(ww[k]), g1 = a2_group_sum(ww[k + 1u]);
        wide |= g0 | g1;
        acc += g0 + g1;
    }
    *wide_or = wide;
    const uint32_t s = live ? acc : 0u;
    const uint32_t s1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s, 0x90 /* quad_perm [0,0,1,2] */, 0xf, 0xf, false);
    const uint32_t s2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s, 0x40 /* quad_perm [0,0,0,1] */, 0xf, 0xf, false);
    const uint32_t s3 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s, 0x00 /* quad_perm [0,0,0,0] */, 0xf, 0xf, false);
    const uint32_t excl = rl == 0u ? 0u : rl == 1u ? s1 : rl == 2u ? s1 + s2 : s1 + s2 + s3;
    return f + excl;
}

// ---- marking one pass (up to sixteen blocks of A, a row of four lanes each) into bm for the window [wlo, wlo + wspan] ----
// Same scheme as intersect_dense.hip: (M << gap) | 1 builds the mask of four postings plus the posting before them, one 64-bit
// shift positions it, two ds_or put it into the bitmap; groups wider than 31 docs and lanes that start outside the window are
// placed posting by posting; rows with multi-byte gaps go through the wave decoder.  Exact for any block.
__device__ __forceinline__ void a2_mark_rows(uint32_t *lds_all, uint32_t *bm, const uint8_t *payload, bool rv, uint32_t f, uint32_t q0,
                                             uint32_t q1, const A2Bytes &B, uint32_t wlo, uint32_t wspan, uint32_t rl, uint32_t row) {
    const uint32_t len = rv ? q1 - q0 : 0u;
    const uint32_t myoff = 64u * rl;
    const uint32_t nb = len > myoff ? (len - myoff < 64u ? len - myoff : 64u) : 0u;
    uint32_t ww[16];
    const unsigned long long hm = a2_prep(B, rv, len, rl, ww);
    auto setbit = [&](uint32_t id, bool valid) {                       // exact range test: any id, any gap
        const uint32_t d = id - wlo;
        if (valid && d <= wspan) atomicOr(&bm[(d + A2_GU) >> 5], 1u << ((d + A2_GU) & 31u));
    };
    if (hm != 0ull) {
#pragma unroll 1
        for (uint32_t r = 0; r < A2_ROWS; r++) {
            if (((hm >> (4u * r)) & 0xFull) == 0ull) continue;
            const uint32_t fq = (uint32_t)__builtin_amdgcn_readlane((int)f, (int)(4u * r)), q0r = (uint32_t)__builtin_amdgcn_readlane((int)q0, (int)(4u * r)),
                           q1r = (uint32_t)__builtin_amdgcn_readlane((int)q1, (int)(4u * r));
            decode_block_wave4(GlobalBytes{payload}, q0r, q1r, fq,
                               [&](uint32_t, uint32_t id0, uint32_t id1, uint32_t id2, uint32_t id3, uint32_t mask) {
                                   setbit(id0, mask & 1u); setbit(id1, mask & 2u); setbit(id2, mask & 4u); setbit(id3, mask & 8u);
                               });
        }
    }
    const bool rowhard = ((hm >> (4u * row)) & 0xFull) != 0ull;
    const bool live = rv && !rowhard;
    uint32_t wide;
    const uint32_t base = a2_lane_base(ww, live, f, rl, &wide);         // id of the posting right before my bytes
    const uint32_t u = base - wlo + A2_GU;                               // its (guard-shifted) position, mod 2^32
    // A lane whose groups of four postings all span < 32 docs spans < 512 docs in all: if it starts outside
    // [wlo - GU, wlo + wspan] it lies wholly outside the window and is skipped.  A lane with a wider group is kept
    // whatever its start; when it starts outside that range every one of its groups is placed posting by posting.
    const bool inrange = u <= wspan + A2_GU;
    const bool haswide = wide >= 32u;
    const bool act = live && (inrange || haswide);
    const bool exactlane = haswide && !inrange;
    const uint32_t lim = wspan + 2u * A2_GU - 64u;                       // a position in the upper guard: where out-of-window groups are parked
    const uint32_t bmbits = (uint32_t)(bm - lds_all) * 32u;              // the bitmap's place inside the workgroup's LDS array, folded into the position
    if (__ballot(act && haswide) == 0ull) {
        // the usual pass: every lane that marks starts inside [wlo - GU, wlo + wspan] and spans < 512 docs, so no group needs
        // the clamp, the wide-group test or the second loop (the bitmap's upper guard holds 512 + 32 bits past the window)
        if (act) {
            uint32_t q = u + bmbits;
#pragma unroll
            for (uint32_t k = 0; k < 16u; k++) {
                const uint32_t x = ww[k];
                uint32_t M = (1u << ((x >> 24) & 31u)) | 1u;
                M = (M << ((x >> 16) & 31u)) | 1u;
                M = (M << ((x >> 8) & 31u)) | 1u;
                M = (M << (x & 31u)) | 1u;                               // bit 0: the posting before the group
                uint32_t *dst = lds_all + (q >> 5);
                const unsigned long long m64 = (unsigned long long)M << (q & 31u);
                atomicOr(dst, (uint32_t)m64);
                atomicOr(dst + 1, (uint32_t)(m64 >> 32));
                q += a2_group_sum(x);
            }
        }
        return;
    }
    if (act) {
        uint32_t q = u + bmbits;
        const uint32_t limb = lim + bmbits;
#pragma unroll
        for (uint32_t k = 0; k < 16u; k++) {
            const uint32_t x = ww[k];
            const uint32_t gs = a2_group_sum(x);
            const bool isw = exactlane || gs >= 32u;                     // the four gaps do not fit one 32-bit mask: placed by the loop below
            uint32_t M = (1u << ((x >> 24) & 31u)) | 1u;
            M = (M << ((x >> 16) & 31u)) | 1u;
            M = (M << ((x >> 8) & 31u)) | 1u;
            M = (M << (x & 31u)) | 1u;                                   // bit 0: the posting before the group
            M = isw ? 0u : M;
            const uint32_t qc = q < limb ? q : limb;                     // groups beyond the window: harmless bits in the guard
            const uint32_t sh = qc & 31u;
            uint32_t *dst = lds_all + (qc >> 5);
            const unsigned long long m64 = (unsigned long long)M << sh;    // (one 64-bit shift: both words)
            atomicOr(dst, (uint32_t)m64);
            atomicOr(dst + 1, (uint32_t)(m64 >> 32));                    // the part that spills into the next word (0 for most)
            q += gs;
        }
    }
    if (__ballot(act && haswide) != 0ull) {
        uint32_t prev = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 16u; k++) {
            const uint32_t gs = a2_group_sum(ww[k]);
            const bool isw = act && haswide && (exactlane || gs >= 32u);
            if (__ballot(isw) != 0ull) {
                if (isw) {
                    const uint32_t x = ww[k];
                    uint32_t d = u + prev - A2_GU;                       // doc - wlo of the posting before the group (mod 2^32)
                    if (k == 0u && rl == 0u && d <= wspan) atomicOr(&bm[(d + A2_GU) >> 5], 1u << ((d + A2_GU) & 31u));   // the block's first doc
#pragma unroll
                    for (uint32_t j = 0; j < 4u; j++) {
                        d += (x >> (8u * j)) & 0xFFu;
                        if (4u * k + j < nb && d <= wspan) atomicOr(&bm[(d + A2_GU) >> 5], 1u << ((d + A2_GU) & 31u));
                    }
                }
            }
            prev += gs;
        }
    }
}

// What both kernels derive, identically, from a wave's sixteen B blocks: the lane's bytes, which rows are hard, the id before
// the lane's bytes and which of the lane's 64 postings exist.
struct A2Lane {
    uint32_t ww[16];
    unsigned long long hm;       // ballot of the hard rows' lanes (wave-uniform)
    bool live;                   // my row has a block of one-byte gaps
    uint32_t base;               // id of the posting right before my bytes (live lanes)
    unsigned long long valid;    // bit j: posting 64 rl + j of my row's block exists (live lanes; 0 otherwise)
};
__device__ __forceinline__ void a2_lane_setup(A2Lane &L, const A2Bytes &B, bool rv, const uint4 &E, uint32_t rl, uint32_t row) {
    uint32_t q1 = E.w;
    asm volatile("" : "+v"(q1));            // (opaque: everything below stays where the call is — hoisted above the marking passes it would hold registers there)
    const uint32_t len = rv ? q1 - E.y : 0u;
    L.hm = a2_prep(B, rv, len, rl, L.ww);
    const bool rowhard = ((L.hm >> (4u * row)) & 0xFull) != 0ull;
    L.live = rv && !rowhard;
    uint32_t wide;
    L.base = a2_lane_base(L.ww, L.live, E.x, rl, &wide);
    // a live row's block is full (256 postings): mine are 64 rl ... 64 rl + 63 — the one before my bytes, then my bytes 0..62
    L.valid = L.live ? ~0ull : 0ull;
}

template <bool RANGE>
__device__ __forceinline__ unsigned long long a2_test_lane(const uint32_t *lds_all, uint32_t bmbits, const A2Lane &L, uint32_t wlo, uint32_t wspan) {
    // u = bit position, inside the workgroup's LDS array, of the posting before my bytes (guard shift and the bitmap's own offset
    // folded in once); lanes without a block probe the window's first bit.  Per posting: one add (the gap byte selected by SDWA),
    // shift + mask for the word's address, the LDS read, one bit-field extract, one shift-or into the answer word.
    const uint32_t org = A2_GU + bmbits;
    uint32_t u = (L.live ? L.base - wlo : 0u) + org;
    uint32_t hlo = 0, hhi = 0;
    auto probe = [&](uint32_t j) {
        uint32_t uu = u;
        bool in = true;
        if (RANGE) { in = u - org <= wspan; uu = in ? u : org; }
        const uint32_t wd = lds_all[uu >> 5];
        uint32_t hit = __builtin_amdgcn_ubfe(wd, uu, 1u);           // (the offset operand is taken mod 32)
        if (RANGE) hit = in ? hit : 0u;
        if (j < 32u) hlo |= hit << j; else hhi |= hit << (j - 32u);
    };
    probe(0u);
#pragma unroll
    for (uint32_t k = 0; k < 63u; k++) {
        u += (L.ww[k >> 2] >> (8u * (k & 3u))) & 0xFFu;
        probe(k + 1u);
    }
    return (((unsigned long long)hhi << 32) | hlo) & L.valid;
}

// a2_test_lane<true> as a loop of sixteen rounds of four postings - the lane's words rotate through ww[0] and are back in place at
// the end.  For a caller short of registers (unrolled, the compiler starts all 64 reads and keeps 64 conditions beside them) on a
// path it rarely takes: a tile wider than one window
__device__ __forceinline__ unsigned long long a2_test_lane_rolled(const uint32_t *lds_all, uint32_t bmbits, A2Lane &L, uint32_t wlo, uint32_t wspan) {
    const uint32_t org = A2_GU + bmbits;
    uint32_t u = (L.live ? L.base - wlo : 0u) + org;
    unsigned long long h = 0ull;
    auto probe = [&](uint32_t j) {
        const bool in = u - org <= wspan;
        const uint32_t uu = in ? u : org;
        const uint32_t wd = lds_all[uu >> 5];
        const uint32_t hit = in ? __builtin_amdgcn_ubfe(wd, uu, 1u) : 0u;           // (the offset operand is taken mod 32)
        h |= (unsigned long long)hit << j;
    };
    probe(0u);
#pragma unroll 1
    for (uint32_t r = 0; r < 16u; r++) {
        const uint32_t x = L.ww[0];
#pragma unroll
        for (uint32_t b = 0; b < 4u; b++) {
            if (4u * r + b < 63u) {                                   // (63 gap bytes: the row's last lane has zeroed its 64th)
                u += (x >> (8u * b)) & 0xFFu;
                probe(4u * r + b + 1u);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 15u; k++) L.ww[k] = L.ww[k + 1u];
        L.ww[15] = x;
    }
    return h & L.valid;
}

// the hard rows of B (multi-byte gaps, a short last block): decoded by the whole wave, every posting inside the window probes the
// bitmap bm and answers by its index in its block (hs: 256 bits per row)
__device__ __forceinline__ void a2_test_hard(const ListView &LB, const uint4 &EB, unsigned long long hm, const uint32_t *bm, uint32_t *hs, uint32_t wlo,
                                             uint32_t wspan) {
#pragma unroll 1
    for (uint32_t r = 0; r < A2_ROWS; r++) {
        if (((hm >> (4u * r)) & 0xFull) == 0ull) continue;
        const uint32_t fq = (uint32_t)__builtin_amdgcn_readlane((int)EB.x, (int)(4u * r)), q0r = (uint32_t)__builtin_amdgcn_readlane((int)EB.y, (int)(4u * r)),
                       q1r = (uint32_t)__builtin_amdgcn_readlane((int)EB.w, (int)(4u * r));
        uint32_t *hr = hs + 8u * r;
        auto probe = [&](uint32_t ix, uint32_t id) {
            const uint32_t d = id - wlo;
            if (d <= wspan && ix < 256u) {
                const uint32_t u = d + A2_GU;
                if ((bm[u >> 5] >> (u & 31u)) & 1u) atomicOr(&hr[ix >> 5], 1u << (ix & 31u));
            }
        };
        decode_block_wave4(GlobalBytes{LB.payload}, q0r, q1r, fq,
                           [&](uint32_t ix, uint32_t id0, uint32_t id1, uint32_t id2, uint32_t id3, uint32_t mask) {
                               if (mask & 1u) { probe(ix, id0); ix++; }
                               if (mask & 2u) { probe(ix, id1); ix++; }
                               if (mask & 4u) { probe(ix, id2); ix++; }
                               if (mask & 8u) { probe(ix, id3); ix++; }
                           });
    }
}

// ---- kernel 1: mark A, test B, one answer bit per B posting -------------------------------------------------------
__device__ __forceinline__ void and2_tiles_body(const DenseParams &p) {
    __shared__ __align__(16) uint32_t lds[4][A2_WAVE_LDS];
    __shared__ uint32_t wcnt[4];
    const int l = lane_id();
    const uint32_t wv = a2_uni(threadIdx.x >> 6);
    const uint32_t rl = (uint32_t)l & 3u, row = (uint32_t)l >> 2;
    const uint32_t w = blockIdx.x * 4u + wv;                 // this wave's number in doc order
    uint32_t *lds_all = &lds[0][0];
    uint32_t *bmA = lds[wv], *hs = bmA + A2_NW;
    const uint32_t bmbits = (uint32_t)(bmA - lds_all) * 32u;
    const ListView LB = p.lists[0], LA = p.lists[1];
    const uint32_t b0 = w * A2_ROWS;
    const uint32_t b1 = b0 + A2_ROWS < LB.nblk ? b0 + A2_ROWS : LB.nblk;
    uint32_t count = 0, lo_w = 0, hi_w = 0, flags = 0;
    unsigned long long H = 0ull;
    unsigned long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tprev = 0;
    const bool stamps = p.debug != nullptr && !p.debug_expand;
#define II2_STAMP(i)                                                    \
    if (stamps) {                                                       \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");              \
        const unsigned long long tn_ = __builtin_amdgcn_s_memtime();    \
        tacc[i] += tn_ - tprev;                                         \
        tprev = tn_;                                                    \
    }
    if (stamps) tprev = __builtin_amdgcn_s_memtime();

    if (b0 < b1) {                                           // wave-uniform
        const uint32_t nvB = b1 - b0;
        const bool rvB = row < nvB;
        const uint4 EB = a2_ent_load(LB, b0, row);
        const uint32_t b_last = a2_uni(*LB.last_doc);
        const uint32_t lo = a2_uni(EB.x);                                       // (row 0 = block b0)
        const uint32_t nf = (uint32_t)__builtin_amdgcn_readlane((int)EB.z, (int)(4u * (nvB - 1u)));
        const uint32_t hi = b1 < LB.nblk ? nf - 1u : b_last;
        lo_w = lo; hi_w = hi;
        // where A enters this wave's doc range: the last block that starts at or before lo.  One probe of 64 entries around
        // a linear guess first (the lists of a dense query are close to uniform: it nearly always brackets the answer and
        // costs one memory round trip instead of three); the full search otherwise
        uint32_t a0;
        {
            const uint32_t fj = p.first_doc[1], lj = p.last_doc[1];
            uint32_t ub = 0xFFFFFFFFu;
            if (LA.nblk > 64u && lj > fj) {
                const uint64_t rel = lo > fj ? (uint64_t)(lo - fj) : 0ull;
                uint64_t gss = rel * LA.nblk / ((uint64_t)(lj - fj) + 1ull);
                if (gss > LA.nblk) gss = LA.nblk;
                uint32_t wb = gss > 32ull ? (uint32_t)gss - 32u : 0u;
                if (wb + 64u > LA.nblk) wb = LA.nblk - 64u;
                const uint32_t fdoc = LA.skip[wb + (uint32_t)l].first_doc;
                const uint32_t cnt = (uint32_t)__popcll(__ballot(fdoc <= lo));   // first docs ascend: the matches are a prefix
                if ((cnt > 0u || wb == 0u) && (cnt < 64u || wb + 64u == LA.nblk)) ub = wb + cnt;
            }
            if (ub == 0xFFFFFFFFu) ub = a2_skip_upper_bound(LA.skip, LA.nblk, lo);
            ub = a2_uni(ub);
            a0 = ub ? ub - 1u : 0u;
        }
        II2_STAMP(0)          // prologue: B's entries, search

        uint32_t wlo = lo & ~31u;
        uint32_t a_cur = a0;
        bool first_window = true;
        unsigned long long hm_any = 0ull;
        for (;;) {
            const uint32_t wspan = hi - wlo < A2_CAPW ? hi - wlo : A2_CAPW - 1u;
            const uint32_t whi = wlo + wspan;
            const uint32_t nw = (wspan >> 5) + 1u;
            const uint32_t ncl = nw + 2u * (A2_GU / 32u) + 2u;       // <= A2_NW - 2; cleared in 4-word steps
            // ---- A's passes over this window.  The entries of the first two passes are requested together; pass k is marked
            // while the payload of pass k + 1 is in flight — and behind A's LAST pass it is B's payload (and the window's
            // tombstone words) that is in flight: B's bytes only take registers once A's are nearly done with theirs.
            uint32_t cur = a_cur;
            uint4 Ecur = a2_ent_load(LA, cur, row), Enext = a2_ent_load(LA, cur + A2_ROWS, row);
            for (uint32_t i = 4u * (uint32_t)l; i < ncl; i += 256u) *reinterpret_cast<uint4 *>(&bmA[i]) = make_uint4(0, 0, 0, 0);
            bool rv = cur + row < LA.nblk && Ecur.x <= whi;          // first docs ascend: the valid rows are a prefix
            uint32_t nv = (uint32_t)__popcll(__ballot(rv)) >> 2;
            A2Bytes Bcur = a2_fetch(LA.payload, rv, Ecur.y, Ecur.w, rl);
            A2Bytes X;
            uint32_t tw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            II2_STAMP(1)      // clear, A's entries, first fetch
            for (;;) {
                const bool more = nv == A2_ROWS;
                const bool rvn = more && cur + A2_ROWS + row < LA.nblk && Enext.x <= whi;
                const uint32_t nvn = (uint32_t)__popcll(__ballot(rvn)) >> 2;
                const bool last = nvn == 0u;
                X = a2_fetch(last ? LB.payload : LA.payload, last ? rvB : rvn, last ? EB.y : Enext.y, last ? EB.w : Enext.w, rl);
                if (last && p.tomb) {                                // (a window holds <= 512 words: eight per lane, requested together)
                    const uint32_t tw0 = wlo >> 5;
#pragma unroll
                    for (uint32_t k = 0; k < 8u; k++) {
                        const uint32_t i = 64u * k + (uint32_t)l;
                        tw[k] = (i < nw && tw0 + i < p.tomb_nwords) ? p.tomb[tw0 + i] : 0u;
                    }
                }
                if (nv != 0u) a2_mark_rows(lds_all, bmA, LA.payload, rv, Ecur.x, Ecur.y, Ecur.w, Bcur, wlo, wspan, rl, row);
                cur += nv;
                if (last) break;
                Ecur = Enext; Bcur = X; rv = rvn; nv = nvn;
                Enext = a2_ent_load(LA, cur + A2_ROWS, row);
            }
            if (cur > a_cur + 1u) a_cur = cur - 1u;                  // A's last block in the window may reach past it
            II2_STAMP(2)      // mark A
            if (p.tomb) {                                            // removed docs are absent from A: no B posting finds them
#pragma unroll
                for (uint32_t k = 0; k < 8u; k++) {
                    const uint32_t i = 64u * k + (uint32_t)l;
                    if (64u * k < nw && tw[k] != 0u) bmA[A2_GU / 32u + i] &= ~tw[k];
                }
            }
            II2_STAMP(3)      // tombstones
            // ---- B's postings against the bitmap
            A2Lane LN;
            a2_lane_setup(LN, X, rvB, EB, rl, row);
            hm_any = LN.hm;
            if (LN.hm != 0ull && first_window) {                     // answers of the hard rows are collected in LDS
                hs[2 * l] = 0u; hs[2 * l + 1] = 0u;
                flags |= 2u;
            }
            const bool single = first_window && hi - wlo < A2_CAPW;
            if (single) H |= a2_test_lane<false>(lds_all, bmbits, LN, wlo, wspan);
            else H |= a2_test_lane<true>(lds_all, bmbits, LN, wlo, wspan);
            if (LN.hm != 0ull) {
#pragma unroll 1
                for (uint32_t r = 0; r < A2_ROWS; r++) {
                    if (((LN.hm >> (4u * r)) & 0xFull) == 0ull) continue;
                    const uint32_t fq = (uint32_t)__builtin_amdgcn_readlane((int)EB.x, (int)(4u * r)), q0r = (uint32_t)__builtin_amdgcn_readlane((int)EB.y, (int)(4u * r)),
                                   q1r = (uint32_t)__builtin_amdgcn_readlane((int)EB.w, (int)(4u * r));
                    uint32_t *hr = hs + 8u * r;
                    auto probe = [&](uint32_t ix, uint32_t id) {
                        const uint32_t d = id - wlo;
                        if (d <= wspan && ix < 256u) {
                            const uint32_t u = d + A2_GU;
                            if ((bmA[u >> 5] >> (u & 31u)) & 1u) atomicOr(&hr[ix >> 5], 1u << (ix & 31u));
                        }
                    };
                    decode_block_wave4(GlobalBytes{LB.payload}, q0r, q1r, fq,
                                       [&](uint32_t ix, uint32_t id0, uint32_t id1, uint32_t id2, uint32_t id3, uint32_t mask) {
                                           if (mask & 1u) { probe(ix, id0); ix++; }
                                           if (mask & 2u) { probe(ix, id1); ix++; }
                                           if (mask & 4u) { probe(ix, id2); ix++; }
                                           if (mask & 8u) { probe(ix, id3); ix++; }
                                       });
                }
            }
            II2_STAMP(4)      // test B
            if (hi - wlo < A2_CAPW) break;
            wlo += A2_CAPW;
            first_window = false;
        }
        if (hm_any != 0ull) {
            const bool rowhard = ((hm_any >> (4u * row)) & 0xFull) != 0ull;
            if (rowhard) H = ((unsigned long long)hs[8u * row + 2u * rl + 1u] << 32) | hs[8u * row + 2u * rl];
        }
        if (hi - lo > 0xFFFFu) flags |= 1u;                   // ids do not fit 16-bit offsets from the round's first doc
        count = wave_sum((uint32_t)__popcll(H));
        p.hmask[(size_t)w * 64u + (uint32_t)l] = make_uint2((uint32_t)H, (uint32_t)(H >> 32));
        II2_STAMP(5)          // count + store
    }
    if (stamps && l == 0)
        for (int i = 0; i < 8; i++) atomicAdd(&p.debug[(uint64_t)(blockIdx.x % 2048u) * 8u + i], tacc[i]);
#undef II2_STAMP
    if (l == 0) {
        wcnt[wv] = count;
        if (w < p.n_meta) p.meta[w] = make_uint4(lo_w, hi_w, count, flags);
    }
    __syncthreads();
    if (threadIdx.x == 0) p.wg_sum[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

__global__ __launch_bounds__(256) void k_and2_tiles(DenseParams p) { and2_tiles_body(p); }

// ---- kernel 2: the B postings whose answer bit is set -> the final ascending id array ------------------------------
// Workgroup g re-walks the B blocks of tile workgroup g (same decomposition).  Its output offset = the counts of the
// workgroups before it, summed here by all 256 threads (a few thousand words) — no separate scan launch.
__global__ __launch_bounds__(256) void k_and2_expand(DenseParams p) {
    __shared__ __align__(16) uint16_t stage[4][A2_STAGE];   // ids of a round as offsets from the round's first doc, in output order
    __shared__ uint32_t hsx[4][A2_HS];
    __shared__ unsigned long long wsum[4];
    const int tid = (int)threadIdx.x, l = tid & 63;
    const uint32_t wv = a2_uni((uint32_t)tid >> 6);
    const uint32_t rl = (uint32_t)l & 3u, row = (uint32_t)l >> 2;
    const uint32_t w0 = blockIdx.x * 4u;
    const uint32_t w = w0 + wv;
    const ListView LB = p.lists[0];
    unsigned long long tacc[4] = {0, 0, 0, 0};
    unsigned long long tprev = 0;
    const bool stamps = p.debug != nullptr && p.debug_expand;
#define II2_STAMP(i)                                                    \
    if (stamps) {                                                       \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");              \
        const unsigned long long tn_ = __builtin_amdgcn_s_memtime();    \
        tacc[i] += tn_ - tprev;                                         \
        tprev = tn_;                                                    \
    }
    if (stamps) tprev = __builtin_amdgcn_s_memtime();
    // everything this wave needs from memory is requested before the offset arithmetic
    const uint32_t b0 = w * A2_ROWS;
    const bool has = b0 < LB.nblk;
    const uint32_t b1 = !has ? b0 : (b0 + A2_ROWS < LB.nblk ? b0 + A2_ROWS : LB.nblk);
    const uint32_t nvB = b1 - b0;
    const bool rvB = row < nvB;
    const uint4 m = w < p.n_meta ? p.meta[w] : make_uint4(0, 0, 0, 0);       // {first doc, last doc, ids, flags}
    uint4 EB = make_uint4(0, 0, 0, 0);
    uint2 Hw = make_uint2(0, 0);
    if (has) {
        EB = a2_ent_load(LB, b0, row);
        Hw = p.hmask[(size_t)w * 64u + (uint32_t)l];
    }
    unsigned long long mine = 0;
    for (uint32_t g = (uint32_t)tid; g < blockIdx.x; g += 256u) mine += p.wg_sum[g];
    for (int d = 32; d >= 1; d >>= 1) mine += (unsigned long long)__shfl_xor((long long)mine, d, 64);
    if (l == 0) wsum[wv] = mine;
    uint32_t before = 0;                        // ids of the waves of this workgroup before mine
    for (uint32_t v = 0; v < wv; v++) before += p.meta[w0 + v].z;
    A2Bytes BB;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) BB.g[k] = make_uint4(0, 0, 0, 0);
    if (has && m.z != 0u) BB = a2_fetch(LB.payload, rvB, EB.y, EB.w, rl);
    __syncthreads();
    const unsigned long long off = wsum[0] + wsum[1] + wsum[2] + wsum[3] + before;
    if (blockIdx.x == gridDim.x - 1u && wv == 3u && l == 0) *p.d_count = off + m.z;     // the last wave: the total
    if (!has || m.z == 0u) return;
    II2_STAMP(0)      // prologue: meta, entries, answers, payload, offsets
    const uint32_t tot = m.z;
    const uint32_t lo = m.x;
    const bool wide = (m.w & 1u) != 0u;
    A2Lane LN;
    a2_lane_setup(LN, BB, rvB, EB, rl, row);
    const unsigned long long H = ((unsigned long long)Hw.y << 32) | Hw.x;
    const uint32_t pc = (uint32_t)__popcll(H);
    const uint32_t incl = wave_incl_scan(pc);
    const uint32_t q0 = incl - pc;              // my first id's place among the wave's ids
    const bool fits = off + tot <= p.out_cap;
    II2_STAMP(1)      // lane sums + scan
    uint16_t *st = stage[wv];
    // the easy rows: 64 steps, the same for every lane
    const unsigned long long He = LN.live ? H : 0ull;
    if (!wide) {
        uint32_t q = q0;
        uint32_t v = LN.base - lo;
        if (He & 1ull) { st[q] = (uint16_t)v; q++; }
#pragma unroll
        for (uint32_t k = 0; k < 63u; k++) {
            v += (LN.ww[k >> 2] >> (8u * (k & 3u))) & 0xFFu;
            if ((He >> (k + 1u)) & 1ull) { st[q] = (uint16_t)v; q++; }
        }
    } else {                                    // a round wider than 64k docs (a sparse stretch): ids go out one by one
        uint32_t q = q0;
        uint32_t v = LN.base;
        if ((He & 1ull) && off + q < p.out_cap) p.out[off + q] = v;
        q += (uint32_t)(He & 1ull);
#pragma unroll
        for (uint32_t k = 0; k < 63u; k++) {
            v += (LN.ww[k >> 2] >> (8u * (k & 3u))) & 0xFFu;
            const uint32_t hit = (uint32_t)((He >> (k + 1u)) & 1ull);
            if (hit && off + q < p.out_cap) p.out[off + q] = v;
            q += hit;
        }
    }
    // rows with multi-byte gaps: the answers are by posting index; the wave decodes the block again and every hit ranks itself
    if (LN.hm != 0ull) {
        uint32_t *hx = hsx[wv];
        hx[2 * l] = Hw.x; hx[2 * l + 1] = Hw.y;               // (lane 4 r + rl holds words 2 rl, 2 rl + 1 of row r: index 8 r + 2 rl = 2 l)
#pragma unroll 1
        for (uint32_t r = 0; r < A2_ROWS; r++) {
            if (((LN.hm >> (4u * r)) & 0xFull) == 0ull) continue;
            const uint32_t fq = (uint32_t)__builtin_amdgcn_readlane((int)EB.x, (int)(4u * r)), q0r = (uint32_t)__builtin_amdgcn_readlane((int)EB.y, (int)(4u * r)),
                           q1r = (uint32_t)__builtin_amdgcn_readlane((int)EB.w, (int)(4u * r));
            const uint32_t qrow = (uint32_t)__builtin_amdgcn_readlane((int)q0, (int)(4u * r));
            const uint32_t *hr = hx + 8u * r;
            auto place = [&](uint32_t ix, uint32_t id) {
                if (ix >= 256u) return;
                const uint32_t wd = hr[ix >> 5];
                if (!((wd >> (ix & 31u)) & 1u)) return;
                uint32_t rk = (uint32_t)__popc(wd & ((1u << (ix & 31u)) - 1u));
                for (uint32_t j = 0; j < (ix >> 5); j++) rk += (uint32_t)__popc(hr[j]);
                if (!wide) st[qrow + rk] = (uint16_t)(id - lo);
                else if (off + qrow + rk < p.out_cap) p.out[off + qrow + rk] = id;
            };
            decode_block_wave4(GlobalBytes{LB.payload}, q0r, q1r, fq,
                               [&](uint32_t ix, uint32_t id0, uint32_t id1, uint32_t id2, uint32_t id3, uint32_t mask) {
                                   if (mask & 1u) { place(ix, id0); ix++; }
                                   if (mask & 2u) { place(ix, id1); ix++; }
                                   if (mask & 4u) { place(ix, id2); ix++; }
                                   if (mask & 8u) { place(ix, id3); ix++; }
                               });
        }
    }
    II2_STAMP(2)      // stage
    if (!wide) {
        // written out 16 bytes per lane (wave-private LDS: program order is enough)
        for (uint32_t c = 4u * (uint32_t)l; c < tot; c += 256u) {
            const uint2 pk = *reinterpret_cast<const uint2 *>(&st[c]);
            const uint4 ids = make_uint4(lo + (pk.x & 0xFFFFu), lo + (pk.x >> 16), lo + (pk.y & 0xFFFFu), lo + (pk.y >> 16));
            if (c + 4u <= tot && fits) {
                uint32_t *dst = p.out + off + c;
                __builtin_memcpy(dst, &ids, 16);                    // one 16-byte store, any 4-byte alignment
            } else {
                const uint32_t vv[4] = {ids.x, ids.y, ids.z, ids.w};
                for (uint32_t k = 0; k < 4u; k++)
                    if (c + k < tot && off + c + k < p.out_cap) p.out[off + c + k] = vv[k];
            }
        }
    }
    II2_STAMP(3)      // flush
    if (stamps && l == 0)
        for (int i = 0; i < 4; i++) atomicAdd(&p.debug[(uint64_t)(blockIdx.x % 2048u) * 8u + i], tacc[i]);
#undef II2_STAMP
}


// ---- one launch: mark A, test B, place the ids ---------------------------------------------------------------------
// The two kernels above hand the answers over through HBM and the second one reads B again (entries, payload, answer bits:
// two dependent round trips before its first useful instruction).  Here the wave that found the answers still holds B's
// bytes and H in registers: it stages its ids (16-bit offsets, wave-private LDS, over the bitmap that is dead by then) and
// writes them out once it knows where — the number of ids of all workgroups before its own.
//
// That prefix comes from the look-back of lookback.h (two hops behind the slowest workgroup it depends on; every wait bounded:
// a workgroup that runs out of patience leaves without writing ids and stores the launch's epoch into the error word; the last
// workgroup poisons the count - all ones - if it already sees that word set, but a give-up may come after it looked, so the host
// reads the error word itself and repeats a failed call through the two kernels above).
constexpr uint32_t A2F_STAGE_W = (A2_STAGE + 1u) / 2u;            // stage in words (aliases the bitmap, which is dead by then)
constexpr uint32_t A2F_WAVE_LDS = (A2F_STAGE_W > A2_NW ? A2F_STAGE_W : A2_NW) + A2_HS;
static_assert(A2F_STAGE_W % 4u == 0u, "16-byte alignment of the per-wave LDS regions");

// What every instance does with a tile's answers (below the kernels): H = one bit per posting of the lane, hs = the hard rows'
// answers by posting index, q0 = the lane's first id's place among the wave's `count` ids, off = the wave's place in the output.
__device__ __forceinline__ void a2f_stage(uint16_t *st, const uint32_t *hs, const ListView &LB, const uint4 &EB, const A2Lane &LN, unsigned long long H,
                                          unsigned long long hm_any, uint32_t lo, uint32_t q0);
__device__ __forceinline__ void a2f_flush(const DenseParams &p, const uint16_t *st, const uint32_t *hs, const ListView &LB, const uint4 &EB, const A2Lane &LN,
                                          unsigned long long H, unsigned long long hm_any, uint32_t lo, uint32_t q0, uint32_t count, bool wide,
                                          unsigned long long off);

//
// ABM: lists[1] has a dense form (p.a_bits: one bit per doc, made once per list and cached with the segment's store).  The
// window's words of it ARE the bitmap the marking passes would build: the wave copies them into LDS - no probe of A's skip
// table, none of A's entries or payload, no marking, no clear - and everything from the test of B's postings on is the same code.
template <bool ABM>
__global__ __launch_bounds__(256, 3) void k_and2_fused(DenseParams p) {
    __shared__ __align__(16) uint32_t lds[4][A2F_WAVE_LDS];
    __shared__ uint32_t wcnt[4];
    __shared__ unsigned long long wg_off;
    __shared__ uint32_t wg_err;
    const int l = lane_id();
    const uint32_t wv = a2_uni(threadIdx.x >> 6);
    const uint32_t rl = (uint32_t)l & 3u, row = (uint32_t)l >> 2;
    const uint32_t g = blockIdx.x;
    const uint32_t w = g * 4u + wv;                          // this wave's number in doc order
    uint32_t *lds_all = &lds[0][0];
    uint32_t *bmA = lds[wv], *hs = bmA + (A2F_WAVE_LDS - A2_HS);
    uint16_t *st = reinterpret_cast<uint16_t *>(bmA);
    const uint32_t bmbits = (uint32_t)(bmA - lds_all) * 32u;
    const ListView LB = p.lists[0], LA = p.lists[1];
    const uint32_t b0 = w * A2_ROWS;
    const uint32_t b1 = b0 + A2_ROWS < LB.nblk ? b0 + A2_ROWS : LB.nblk;
    uint32_t count = 0, lo = 0, hi = 0;
    unsigned long long H = 0ull, hm_any = 0ull;
    A2Lane LN;
    uint4 EB = make_uint4(0, 0, 0, 0);
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
    const bool work = b0 < b1;                               // wave-uniform
    const uint32_t nvB = work ? b1 - b0 : 0u;
    const bool rvB = row < nvB;

    if (ABM && work) {
        EB = a2_ent_load(LB, b0, row);
        const uint32_t b_last = a2_uni(*LB.last_doc);
        lo = a2_uni(EB.x);                                                      // (row 0 = block b0)
        const uint32_t nf = (uint32_t)__builtin_amdgcn_readlane((int)EB.z, (int)(4u * (nvB - 1u)));
        hi = b1 < LB.nblk ? nf - 1u : b_last;
        II2_STAMP(0)          // prologue: B's entries
        uint32_t wlo = lo & ~31u;
        bool first_window = true;
        A2Bytes X;
        for (;;) {
            const uint32_t wspan = hi - wlo < A2_CAPW ? hi - wlo : A2_CAPW - 1u;
            const uint32_t nw = (wspan >> 5) + 1u;
            // ---- one round trip: the window's words of A's form (<= 512: eight per lane, coalesced), its tombstone words and -
            // for the first window - B's payload.  wlo and a_origin are multiples of 32: a window maps onto whole words; B's
            // docs may start before A's, end after them or miss them altogether: words outside [0, a_nwords) are 0
            const int32_t aw0 = (int32_t)(wlo >> 5) - (int32_t)(p.a_origin >> 5);
            const uint32_t tw0 = wlo >> 5;
            uint32_t aw[8], tw[8];
#pragma unroll
            for (uint32_t k = 0; k < 8u; k++) {
                const uint32_t i = 64u * k + (uint32_t)l;
                const int32_t ai = aw0 + (int32_t)i;
                aw[k] = (i < nw && ai >= 0 && (uint32_t)ai < p.a_nwords) ? p.a_bits[ai] : 0u;
                tw[k] = (p.tomb && i < nw && tw0 + i < p.tomb_nwords) ? p.tomb[tw0 + i] : 0u;
            }
            if (first_window) X = a2_fetch(LB.payload, rvB, EB.y, EB.w, rl);
            II2_STAMP(1)      // requests: A's words, tombstones, B's payload
            // removed docs are absent from A (no B posting finds them).  The test reads the words [GU/32, GU/32 + nw) only: a live
            // lane's postings lie in [lo, hi], the others' answers are masked - the guards need no clearing
#pragma unroll
            for (uint32_t k = 0; k < 8u; k++)
                if (64u * k < nw) bmA[A2_GU / 32u + 64u * k + (uint32_t)l] = aw[k] & ~tw[k];
            II2_STAMP(2)      // A's words into LDS
            if (first_window) {
                a2_lane_setup(LN, X, rvB, EB, rl, row);
                hm_any = LN.hm;
                if (LN.hm != 0ull) { hs[2 * l] = 0u; hs[2 * l + 1] = 0u; }      // answers of the hard rows are collected in LDS
            }
            const bool single = first_window && hi - wlo < A2_CAPW;
            if (single) H |= a2_test_lane<false>(lds_all, bmbits, LN, wlo, wspan);
            else H |= a2_test_lane<true>(lds_all, bmbits, LN, wlo, wspan);
            if (LN.hm != 0ull) a2_test_hard(LB, EB, LN.hm, bmA, hs, wlo, wspan);
            II2_STAMP(3)      // test B
            if (hi - wlo < A2_CAPW) break;
            wlo += A2_CAPW;
            first_window = false;
        }
        if (hm_any != 0ull) {
            const bool rowhard = ((hm_any >> (4u * row)) & 0xFull) != 0ull;
            if (rowhard) H = ((unsigned long long)hs[8u * row + 2u * rl + 1u] << 32) | hs[8u * row + 2u * rl];
        }
    }
    if (!ABM && work) {
        // ---- first round trip: B's entries and, beside them, a 128-entry window of A's skip table around the place where a
        // uniform list would have this wave's first doc (B's docs-per-block and A's blocks-per-doc from the host: a guess that
        // the entries themselves confirm or refute)
        EB = a2_ent_load(LB, b0, row);
        const uint32_t fj = p.first_doc[1];
        uint32_t wb = 0;
        uint2 P0 = make_uint2(0, 0), P1 = make_uint2(0, 0);
        const bool probing = LA.nblk >= 128u;
        if (probing) {
            const float lo_guess = (float)p.first_doc[0] + (float)b0 * p.b_dpb;
            const float rel = lo_guess - (float)fj;
            float gs = rel > 0.f ? rel * p.a_scale : 0.f;
            if (gs > (float)LA.nblk) gs = (float)LA.nblk;
            const uint32_t gi = (uint32_t)gs;
            wb = gi > 40u ? gi - 40u : 0u;
            if (wb + 128u > LA.nblk) wb = LA.nblk - 128u;
            wb = a2_uni(wb);
            const ii2_skip e0 = LA.skip[wb + (uint32_t)l], e1 = LA.skip[wb + 64u + (uint32_t)l];
            P0 = make_uint2(e0.first_doc, e0.byte_off);
            P1 = make_uint2(e1.first_doc, e1.byte_off);
        }
        const uint32_t b_last = a2_uni(*LB.last_doc);
        lo = a2_uni(EB.x);                                                      // (row 0 = block b0)
        const uint32_t nf = (uint32_t)__builtin_amdgcn_readlane((int)EB.z, (int)(4u * (nvB - 1u)));
        hi = b1 < LB.nblk ? nf - 1u : b_last;
        // where A enters this wave's doc range: the last block that starts at or before lo
        uint32_t a0;
        bool from_probe = false;
        {
            uint32_t ub = 0xFFFFFFFFu;
            if (probing) {
                const uint32_t c0 = (uint32_t)__popcll(__ballot(P0.x <= lo)), c1 = (uint32_t)__popcll(__ballot(P1.x <= lo));   // first docs ascend: the matches are a prefix
                const uint32_t cnt = c0 + c1;
                if ((cnt > 0u || wb == 0u) && (cnt < 128u || wb + 128u == LA.nblk)) { ub = wb + cnt; from_probe = true; }
            }
            if (ub == 0xFFFFFFFFu) ub = a2_skip_upper_bound(LA.skip, LA.nblk, lo);
            ub = a2_uni(ub);
            a0 = ub ? ub - 1u : 0u;
        }
        II2_STAMP(0)          // prologue: B's entries, A's window, search

        uint32_t wlo = lo & ~31u;
        uint32_t a_cur = a0;
        bool first_window = true;
        for (;;) {
            const uint32_t wspan = hi - wlo < A2_CAPW ? hi - wlo : A2_CAPW - 1u;
            const uint32_t whi = wlo + wspan;
            const uint32_t nw = (wspan >> 5) + 1u;
            const uint32_t ncl = nw + 2u * (A2_GU / 32u) + 2u;       // <= A2_NW - 2; cleared in 4-word steps
            uint32_t cur = a_cur;
            uint4 Ecur, Enext;
            // the entries of A's first two passes: out of the window's registers when it holds them (no second round trip)
            if (first_window && from_probe && cur + 2u * A2_ROWS + 1u <= wb + 127u && cur + 2u * A2_ROWS + 1u <= LA.nblk) {
                auto pick = [&](uint32_t j, uint32_t &fd, uint32_t &bo) {      // entry wb + j, j < 128 (per lane)
                    const int src = (int)((j & 63u) << 2);
                    const uint32_t f0 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)P0.x), f1 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)P1.x);
                    const uint32_t o0 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)P0.y), o1 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)P1.y);
                    fd = j < 64u ? f0 : f1;
                    bo = j < 64u ? o0 : o1;
                };
                const uint32_t j0 = cur - wb + row;
                pick(j0, Ecur.x, Ecur.y); pick(j0 + 1u, Ecur.z, Ecur.w);
                pick(j0 + A2_ROWS, Enext.x, Enext.y); pick(j0 + A2_ROWS + 1u, Enext.z, Enext.w);
            } else {
                Ecur = a2_ent_load(LA, cur, row);
                Enext = a2_ent_load(LA, cur + A2_ROWS, row);
            }
            for (uint32_t i = 4u * (uint32_t)l; i < ncl; i += 256u) *reinterpret_cast<uint4 *>(&bmA[i]) = make_uint4(0, 0, 0, 0);
            bool rv = cur + row < LA.nblk && Ecur.x <= whi;          // first docs ascend: the valid rows are a prefix
            uint32_t nv = (uint32_t)__popcll(__ballot(rv)) >> 2;
            A2Bytes Bcur = a2_fetch(LA.payload, rv, Ecur.y, Ecur.w, rl);
            A2Bytes X;
            uint32_t tw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            II2_STAMP(1)      // clear, A's entries, first fetch
            for (;;) {
                const bool more = nv == A2_ROWS;
                const bool rvn = more && cur + A2_ROWS + row < LA.nblk && Enext.x <= whi;
                const uint32_t nvn = (uint32_t)__popcll(__ballot(rvn)) >> 2;
                const bool last = nvn == 0u;
                X = a2_fetch(last ? LB.payload : LA.payload, last ? rvB : rvn, last ? EB.y : Enext.y, last ? EB.w : Enext.w, rl);
                if (last && p.tomb) {                                // (a window holds <= 512 words: eight per lane, requested together)
                    const uint32_t tw0 = wlo >> 5;
#pragma unroll
                    for (uint32_t k = 0; k < 8u; k++) {
                        const uint32_t i = 64u * k + (uint32_t)l;
                        tw[k] = (i < nw && tw0 + i < p.tomb_nwords) ? p.tomb[tw0 + i] : 0u;
                    }
                }
                if (nv != 0u) a2_mark_rows(lds_all, bmA, LA.payload, rv, Ecur.x, Ecur.y, Ecur.w, Bcur, wlo, wspan, rl, row);
                cur += nv;
                if (last) break;
                Ecur = Enext; Bcur = X; rv = rvn; nv = nvn;
                Enext = a2_ent_load(LA, cur + A2_ROWS, row);
            }
            if (cur > a_cur + 1u) a_cur = cur - 1u;                  // A's last block in the window may reach past it
            II2_STAMP(2)      // mark A
            if (p.tomb) {                                            // removed docs are absent from A: no B posting finds them
#pragma unroll
                for (uint32_t k = 0; k < 8u; k++) {
                    const uint32_t i = 64u * k + (uint32_t)l;
                    if (64u * k < nw && tw[k] != 0u) bmA[A2_GU / 32u + i] &= ~tw[k];
                }
            }
            // ---- B's postings against the bitmap
            a2_lane_setup(LN, X, rvB, EB, rl, row);
            hm_any = LN.hm;
            if (LN.hm != 0ull && first_window) { hs[2 * l] = 0u; hs[2 * l + 1] = 0u; }      // answers of the hard rows are collected in LDS
            const bool single = first_window && hi - wlo < A2_CAPW;
            if (single) H |= a2_test_lane<false>(lds_all, bmbits, LN, wlo, wspan);
            else H |= a2_test_lane<true>(lds_all, bmbits, LN, wlo, wspan);
            if (LN.hm != 0ull) {
#pragma unroll 1
                for (uint32_t r = 0; r < A2_ROWS; r++) {
                    if (((LN.hm >> (4u * r)) & 0xFull) == 0ull) continue;
                    const uint32_t fq = (uint32_t)__builtin_amdgcn_readlane((int)EB.x, (int)(4u * r)), q0r = (uint32_t)__builtin_amdgcn_readlane((int)EB.y, (int)(4u * r)),
                                   q1r = (uint32_t)__builtin_amdgcn_readlane((int)EB.w, (int)(4u * r));
                    uint32_t *hr = hs + 8u * r;
                    auto probe = [&](uint32_t ix, uint32_t id) {
                        const uint32_t d = id - wlo;
                        if (d <= wspan && ix < 256u) {
                            const uint32_t u = d + A2_GU;
                            if ((bmA[u >> 5] >> (u & 31u)) & 1u) atomicOr(&hr[ix >> 5], 1u << (ix & 31u));
                        }
                    };
                    decode_block_wave4(GlobalBytes{LB.payload}, q0r, q1r, fq,
                                       [&](uint32_t ix, uint32_t id0, uint32_t id1, uint32_t id2, uint32_t id3, uint32_t mask) {
                                           if (mask & 1u) { probe(ix, id0); ix++; }
                                           if (mask & 2u) { probe(ix, id1); ix++; }
                                           if (mask & 4u) { probe(ix, id2); ix++; }
                                           if (mask & 8u) { probe(ix, id3); ix++; }
                                       });
                }
            }
            II2_STAMP(3)      // tombstones, test B
            if (hi - wlo < A2_CAPW) break;
            wlo += A2_CAPW;
            first_window = false;
        }
        if (hm_any != 0ull) {
            const bool rowhard = ((hm_any >> (4u * row)) & 0xFull) != 0ull;
            if (rowhard) H = ((unsigned long long)hs[8u * row + 2u * rl + 1u] << 32) | hs[8u * row + 2u * rl];
        }
    }
    const uint32_t pc = (uint32_t)__popcll(H);
    const uint32_t incl = wave_incl_scan(pc);
    count = wave_bcast(incl, 63);
    const uint32_t q0 = incl - pc;              // my first id's place among the wave's ids
    if (l == 0) wcnt[wv] = count;
    lds_barrier();
    const uint32_t c0 = wcnt[0], c1 = wcnt[1], c2 = wcnt[2], c3 = wcnt[3];
    const uint32_t total = c0 + c1 + c2 + c3;
    const uint32_t before = wv == 0u ? 0u : wv == 1u ? c0 : wv == 2u ? c0 + c1 : c0 + c1 + c2;
    if (threadIdx.x == 0) lb_publish(p.lb, g, total);
    II2_STAMP(4)              // count, barrier, publish
    if (wv == 1u && lb_is_leader(g, gridDim.x)) {            // the group's ids, as soon as its other members have published theirs
        if (!lb_group_publish(p.lb, g, total) && l == 0) { wg_err = 1u; lb_fail(p.lb); }
    }
    // ---- stage the ids of my postings whose answer bit is set: 16-bit offsets from the round's first doc, in output order
    const bool wide = work && hi - lo > 0xFFFFu;             // (a sparse stretch: ids go out one by one, by the flush)
    if (work && !wide && count != 0u) a2f_stage(st, hs, LB, EB, LN, H, hm_any, lo, q0);
    II2_STAMP(5)              // stage
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
    II2_STAMP(6)              // look-back
    lds_barrier();
    const bool err = wg_err != 0u;
    const unsigned long long off = wg_off + before;
    if (g == gridDim.x - 1u && threadIdx.x == 0) {          // the last workgroup: the total, or all ones when some workgroup gave up
        const bool anyerr = err || lb_failed(p.lb);
        *p.d_count = anyerr ? ~0ull : wg_off + total;
        if (p.lb.spin == LB_SPIN_LATE) lb_late_done(p.lb);
    }
    if (work && !err && count != 0u) a2f_flush(p, st, hs, LB, EB, LN, H, hm_any, lo, q0, count, wide, off);
    II2_STAMP(7)              // flush
    if (stamps && l == 0)
        for (int i = 0; i < 8; i++) atomicAdd(&p.debug[(uint64_t)(blockIdx.x % 2048u) * 8u + i], tacc[i]);
#undef II2_STAMP
}

// ---- the dense-form instance with TWO tiles per wave ------------------------------------------------------------------
// The life of a wave of k_and2_fused<true> is a chain of waits - B's entries, then A's words and B's payload, then the look-back -
// around little work, and a grid that the device does not hold at once pays that chain once per round of workgroups.  Here
// workgroup g owns the blocks [128 g, 128 g + 128) of B; tile s of wave wv is the sixteen blocks from 128 g + 64 s + 16 wv on
// (output order = doc order: tile 0 of waves 0..3, then tile 1 of waves 0..3), and the chain is paid once for both tiles:
//   * the skip entries of both come in one round trip, and so does everything else: tile 1's requests go out right behind
//     tile 0's, and what they bring waits in LDS - the stage area is dead until both tiles are tested - while tile 0 is tested;
//   * ONE look-back record per workgroup carries the ids of both tiles, published once both are tested (a record per tile would
//     chain the grid: workgroup g - 1 would publish its tile 1 only after its tile 0 had waited for workgroup g - 2);
//   * tile 1's place is the workgroup's plus tile 0's ids - no second look-back - and it is staged while tile 0's stores travel.
// Half the workgroups, each 1.7 times as long (DESIGN.md 4.1a'): launch_intersect_and2 takes this instance when setop.cpp found
// that the one-tile grid does not fit the device at once (DenseParams::and2_tiles).
constexpr uint32_t A2F2_WAVE_LDS = A2F_WAVE_LDS + A2_HS;          // a second answer area: tile 0's hard rows answer until they are staged, after tile 1's test
constexpr uint32_t A2F2_WIN = A2_GU / 32u + A2_CAPW / 32u;        // words of a window of the dense form: the lower guard's place, then <= 512 words (no guard is read)
constexpr uint32_t A2F2_PARK = 2u * A2F2_WIN;                      // tile 1's payload, 64 bytes a lane, waits behind the two windows
static_assert(A2F2_WIN % 4u == 0u && A2F2_PARK + 64u * 16u <= A2F2_WAVE_LDS - A2_HS, "two windows and the parked payload end before tile 0's answer area");

// Words [w0, w0 + nw) of a bit array of n_words (>= 1) words, eight per lane (coalesced), in two steps.  a2f_words_request: every
// lane loads, from an index clamped into the window and into the array - a load under a per-element condition gets a branch of
// its own, behind which the compiler may wait for everything in flight, and a select kept from before the load costs a register
// per word for as long as the load travels.  a2f_words_settle, once they have landed: the words outside the array are zero (B's
// docs may start before A's, end after them or miss them altogether); words past the window are whatever was loaded - nobody
// reads them.  w0 is made opaque in between (A2F_OPAQUE), so that the second step's conditions are worked out there.
#define A2F_OPAQUE(x) asm volatile("" : "+s"(x))
__device__ __forceinline__ void a2f_words_request(const uint32_t *__restrict__ bits, int32_t w0, uint32_t n_words, uint32_t nw, uint32_t (&out)[8]) {
    const uint32_t l = (uint32_t)lane_id();
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++) {
        const uint32_t i = 64u * k + l;
        const int32_t wi = w0 + (int32_t)(i < nw ? i : nw - 1u);
        const uint32_t at = wi < 0 ? 0u : (uint32_t)wi < n_words ? (uint32_t)wi : n_words - 1u;
        // (a 32-bit byte offset from the uniform base - one address register a load, not two: n_words <= 2^27, one bit per doc id)
        out[k] = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(bits) + 4u * at);
    }
}
__device__ __forceinline__ void a2f_words_settle(int32_t w0, uint32_t n_words, uint32_t (&out)[8]) {
    const uint32_t l = (uint32_t)lane_id();
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++) out[k] = (uint32_t)(w0 + (int32_t)(64u * k + l)) < n_words ? out[k] : 0u;      // (below the array: a huge unsigned index)
}

// a2_fetch in the same two steps: every lane loads its four 16-byte pieces - a piece past the block's end from the block's first
// bytes instead, which can always be read (a block ends at or before the payload's end, and segments carry 16 bytes of padding) -
// and zeroes those pieces afterwards (q1 made opaque in between)
__device__ __forceinline__ A2Bytes a2f_fetch_request(const uint8_t *payload, bool rv, uint32_t q0, uint32_t q1, uint32_t rl) {
    const uint32_t len = rv ? q1 - q0 : 0u;
    A2Bytes B;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t off = 64u * rl + 16u * k;
        __builtin_memcpy(&B.g[k], payload + (q0 + (len > off ? off : 0u)), 16);      // (a 32-bit offset from the uniform base)
    }
    return B;
}
__device__ __forceinline__ void a2f_fetch_settle(A2Bytes &B, bool rv, uint32_t q0, uint32_t q1, uint32_t rl) {
    const uint32_t len = rv ? q1 - q0 : 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++)
        if (!(len > 64u * rl + 16u * k)) B.g[k] = make_uint4(0, 0, 0, 0);
}

// A's words of a window - the removed docs are out of them already (absent from A: no B posting finds them) - into the wave's LDS
// window.  The test reads the words [GU/32, GU/32 + nw) only: a live lane's postings lie in [lo, hi], the others' answers are masked
__device__ __forceinline__ void a2f_window_store(uint32_t *bmA, const uint32_t (&aw)[8], uint32_t nw) {
    const uint32_t l = (uint32_t)lane_id();
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++)
        if (64u * k < nw) bmA[A2_GU / 32u + 64u * k + l] = aw[k];
}

// a tile's postings against A's words, window by window (the first window is in LDS already; windows behind it - a tile wider
// than A2_CAPW docs - are loaded here, one round trip each): one answer bit per posting of the lane
__device__ __forceinline__ unsigned long long a2f_probe(const DenseParams &p, const ListView &LB, uint32_t *lds_all, uint32_t *bmA, uint32_t *hs,
                                                        A2Lane &LN, const uint4 &EB, uint32_t lo, uint32_t hi, uint32_t rl, uint32_t row) {
    const uint32_t bmbits = (uint32_t)(bmA - lds_all) * 32u;
    uint32_t wlo = lo & ~31u;
    unsigned long long H = 0ull;
    if (hi - wlo < A2_CAPW) {
        H = a2_test_lane<false>(lds_all, bmbits, LN, wlo, hi - wlo);
        if (LN.hm != 0ull) a2_test_hard(LB, EB, LN.hm, bmA, hs, wlo, hi - wlo);
    } else {
#pragma unroll 1
        for (;;) {
            const uint32_t wspan = hi - wlo < A2_CAPW ? hi - wlo : A2_CAPW - 1u;
            H |= a2_test_lane_rolled(lds_all, bmbits, LN, wlo, wspan);
            if (LN.hm != 0ull) a2_test_hard(LB, EB, LN.hm, bmA, hs, wlo, wspan);
            if (hi - wlo < A2_CAPW) break;
            wlo += A2_CAPW;
            const uint32_t nw = ((hi - wlo < A2_CAPW ? hi - wlo : A2_CAPW - 1u) >> 5) + 1u;
            const int32_t wa = (int32_t)(wlo >> 5) - (int32_t)(p.a_origin >> 5), wt = (int32_t)(wlo >> 5);
            uint32_t aw[8];
            a2f_words_request(p.a_bits, wa, p.a_nwords, nw, aw);
            a2f_words_settle(wa, p.a_nwords, aw);
            if (p.tomb && p.tomb_nwords) {
                uint32_t tw[8];
                a2f_words_request(p.tomb, wt, p.tomb_nwords, nw, tw);
                a2f_words_settle(wt, p.tomb_nwords, tw);
#pragma unroll
                for (uint32_t k = 0; k < 8u; k++) aw[k] &= ~tw[k];
            }
            a2f_window_store(bmA, aw, nw);
        }
    }
    if (LN.hm != 0ull) {
        const bool rowhard = ((LN.hm >> (4u * row)) & 0xFull) != 0ull;
        if (rowhard) H = ((unsigned long long)hs[8u * row + 2u * rl + 1u] << 32) | hs[8u * row + 2u * rl];
    }
    return H;
}

__global__ __launch_bounds__(256, 4) void k_and2_fused_x2(DenseParams p) {
    __shared__ __align__(16) uint32_t lds[4][A2F2_WAVE_LDS];
    __shared__ uint32_t wcnt[2][4];
    __shared__ unsigned long long wg_off;
    __shared__ uint32_t wg_err;
    const int l = lane_id();
    const uint32_t wv = a2_uni(threadIdx.x >> 6);
    const uint32_t rl = (uint32_t)l & 3u, row = (uint32_t)l >> 2;
    const uint32_t g = blockIdx.x;
    uint32_t *lds_all = &lds[0][0];
    // a wave's LDS: [tile 0's window | tile 1's window | tile 1's parked payload ...) until both tiles are tested, the stage
    // after that; behind them the hard rows' answers of tile 1 - the parked payload ends in there, and is gone before they are
    // cleared - and of tile 0
    uint32_t *bmA = lds[wv], *bmA1 = bmA + A2F2_WIN, *park = bmA + A2F2_PARK;
    uint32_t *hs1 = bmA + (A2F2_WAVE_LDS - 2u * A2_HS), *hs0 = hs1 + A2_HS;
    uint16_t *st = reinterpret_cast<uint16_t *>(bmA);
    const ListView LB = p.lists[0];
    // tile 0 / tile 1 of this wave: first block, valid rows
    const uint32_t b0 = (g * 8u + wv) * A2_ROWS, b1 = b0 + 4u * A2_ROWS;
    const uint32_t nv0 = b0 < LB.nblk ? (LB.nblk - b0 < A2_ROWS ? LB.nblk - b0 : A2_ROWS) : 0u;
    const uint32_t nv1 = b1 < LB.nblk ? (LB.nblk - b1 < A2_ROWS ? LB.nblk - b1 : A2_ROWS) : 0u;
    const bool work0 = nv0 != 0u, work1 = nv1 != 0u;         // wave-uniform; tile 1 has work only where tile 0 has
    const bool rv0 = row < nv0, rv1 = row < nv1;
    uint32_t lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0;
    unsigned long long H0 = 0ull, H1 = 0ull;
    A2Lane LN0, LN1;
    uint4 E0 = make_uint4(0, 0, 0, 0), E1 = make_uint4(0, 0, 0, 0);
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

    if (work0) {
        // ---- one round trip: the skip entries of both tiles (they depend on the wave's number only; a tile without blocks reads
        // the list's end entry)
        E0 = a2_ent_load(LB, b0, row);
        E1 = a2_ent_load(LB, b1, row);
        const uint32_t b_last = a2_uni(*LB.last_doc);
        lo0 = a2_uni(E0.x);                                                     // (row 0 = the tile's first block)
        hi0 = b0 + A2_ROWS < LB.nblk ? (uint32_t)__builtin_amdgcn_readlane((int)E0.z, (int)(4u * (nv0 - 1u))) - 1u : b_last;
        if (work1) {
            lo1 = a2_uni(E1.x);
            hi1 = b1 + A2_ROWS < LB.nblk ? (uint32_t)__builtin_amdgcn_readlane((int)E1.z, (int)(4u * (nv1 - 1u))) - 1u : b_last;
        }
        asm volatile("" : : "v"(E0.y), "v"(E0.w), "v"(E1.y), "v"(E1.w));       // (every entry is waited for here: no such wait is left to fall among the requests)
        II2_STAMP(0)          // prologue: B's entries, both tiles
        // ---- one go: the first window's words of A's form and the tombstone words, of tile 0 and of tile 1, then B's payload of
        // tile 0 and of tile 1 - forty loads a lane, one round trip
        const bool tombs = p.tomb != nullptr && p.tomb_nwords != 0u;
        const uint32_t wl0 = lo0 & ~31u, wl1 = lo1 & ~31u;
        const uint32_t nw0 = ((hi0 - wl0 < A2_CAPW ? hi0 - wl0 : A2_CAPW - 1u) >> 5) + 1u;
        const uint32_t nw1 = ((hi1 - wl1 < A2_CAPW ? hi1 - wl1 : A2_CAPW - 1u) >> 5) + 1u;
        int32_t wa0 = (int32_t)(wl0 >> 5) - (int32_t)(p.a_origin >> 5), wa1 = (int32_t)(wl1 >> 5) - (int32_t)(p.a_origin >> 5);
        int32_t wt0 = (int32_t)(wl0 >> 5), wt1 = (int32_t)(wl1 >> 5);
        uint32_t aw0[8], aw1[8], tw0[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tw1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        a2f_words_request(p.a_bits, wa0, p.a_nwords, nw0, aw0);
        a2f_words_request(p.a_bits, wa1, p.a_nwords, nw1, aw1);
        if (tombs) {
            a2f_words_request(p.tomb, wt0, p.tomb_nwords, nw0, tw0);
            a2f_words_request(p.tomb, wt1, p.tomb_nwords, nw1, tw1);
        }
        A2Bytes X0 = a2f_fetch_request(LB.payload, rv0, E0.y, E0.w, rl);
        {
            A2Bytes X1 = a2f_fetch_request(LB.payload, rv1, E1.y, E1.w, rl);
            II2_STAMP(1)      // requests, both tiles
            // ---- landed.  Everything of tile 1 goes into LDS at once - its words into a window of its own, its payload behind
            // that - and waits there, not in twenty-four registers, while tile 0 is tested: the test keeps as many LDS reads in
            // flight as it has registers for, and four waves a SIMD leave it 128.  (Loads come back in the order they went out,
            // within a few hundred cycles of each other: waiting for the last of them here costs little.)
            uint32_t tombs2 = a2_uni(tombs ? 1u : 0u), qe0 = E0.w, qe1 = E1.w;
            A2F_OPAQUE(wa0); A2F_OPAQUE(wa1); A2F_OPAQUE(wt0); A2F_OPAQUE(wt1); A2F_OPAQUE(tombs2);
            asm volatile("" : "+v"(qe0), "+v"(qe1));
            a2f_words_settle(wa0, p.a_nwords, aw0);
            a2f_words_settle(wa1, p.a_nwords, aw1);
            if (tombs2) {                                              // (opaque too, and the words: their complement is not taken - and waited for - among the requests)
#pragma unroll
                for (uint32_t k = 0; k < 8u; k++) asm volatile("" : "+v"(tw0[k]), "+v"(tw1[k]));
                a2f_words_settle(wt0, p.tomb_nwords, tw0);
                a2f_words_settle(wt1, p.tomb_nwords, tw1);
#pragma unroll
                for (uint32_t k = 0; k < 8u; k++) { aw0[k] &= ~tw0[k]; aw1[k] &= ~tw1[k]; }
            }
            a2f_window_store(bmA, aw0, nw0);
            a2f_window_store(bmA1, aw1, nw1);
            a2f_fetch_settle(X0, rv0, E0.y, qe0, rl);
            a2f_fetch_settle(X1, rv1, E1.y, qe1, rl);
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) *reinterpret_cast<uint4 *>(&park[256u * k + 4u * (uint32_t)l]) = X1.g[k];
        }
        a2_lane_setup(LN0, X0, rv0, E0, rl, row);
        if (LN0.hm != 0ull) { hs0[2 * l] = 0u; hs0[2 * l + 1] = 0u; }           // answers of the hard rows are collected in LDS
        II2_STAMP(2)          // A's words and tile 1's payload into LDS
        H0 = a2f_probe(p, LB, lds_all, bmA, hs0, LN0, E0, lo0, hi0, rl, row);
        II2_STAMP(3)          // test B, tile 0
        if (work1) {
            A2Bytes X1;
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) X1.g[k] = *reinterpret_cast<const uint4 *>(&park[256u * k + 4u * (uint32_t)l]);
            a2_lane_setup(LN1, X1, rv1, E1, rl, row);
            if (LN1.hm != 0ull) { hs1[2 * l] = 0u; hs1[2 * l + 1] = 0u; }       // (over the end of the parked payload, which is in registers by now)
            II2_STAMP(2)      // tile 1's payload out of LDS
            H1 = a2f_probe(p, LB, lds_all, bmA1, hs1, LN1, E1, lo1, hi1, rl, row);
            II2_STAMP(3)      // test B, tile 1
        }
    }
    // ---- the ids of both tiles; one record for the workgroup
    const uint32_t pc0 = (uint32_t)__popcll(H0), pc1 = (uint32_t)__popcll(H1);
    const uint32_t in0 = wave_incl_scan(pc0), in1 = wave_incl_scan(pc1);
    const uint32_t count0 = wave_bcast(in0, 63), count1 = wave_bcast(in1, 63);
    const uint32_t q0 = in0 - pc0, q1 = in1 - pc1;          // my first id's place among the wave's ids of the tile
    if (l == 0) { wcnt[0][wv] = count0; wcnt[1][wv] = count1; }
    lds_barrier();
    uint32_t total0 = 0, total1 = 0, before0 = 0, before1 = 0;
#pragma unroll
    for (uint32_t v = 0; v < 4u; v++) {
        const uint32_t c0 = wcnt[0][v], c1 = wcnt[1][v];
        before0 += v < wv ? c0 : 0u; before1 += v < wv ? c1 : 0u;
        total0 += c0; total1 += c1;
    }
    const uint32_t total = total0 + total1;
    if (threadIdx.x == 0) lb_publish(p.lb, g, total);
    II2_STAMP(4)              // count, barrier, publish
    if (wv == 1u && lb_is_leader(g, gridDim.x)) {            // the group's ids, as soon as its other members have published theirs
        if (!lb_group_publish(p.lb, g, total) && l == 0) { wg_err = 1u; lb_fail(p.lb); }
    }
    const bool wide0 = work0 && hi0 - lo0 > 0xFFFFu, wide1 = work1 && hi1 - lo1 > 0xFFFFu;
    if (work0 && !wide0 && count0 != 0u) a2f_stage(st, hs0, LB, E0, LN0, H0, LN0.hm, lo0, q0);
    II2_STAMP(5)              // stage, tile 0
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
    II2_STAMP(6)              // look-back
    lds_barrier();
    const bool err = wg_err != 0u;
    if (g == gridDim.x - 1u && threadIdx.x == 0) {          // the last workgroup: the total, or all ones when some workgroup gave up
        const bool anyerr = err || lb_failed(p.lb);
        *p.d_count = anyerr ? ~0ull : wg_off + total;
        if (p.lb.spin == LB_SPIN_LATE) lb_late_done(p.lb);
    }
    // ---- tile 0 out; tile 1 into the same stage while those stores travel (wave-private LDS: program order is enough), and out
    if (work0 && !err && count0 != 0u) a2f_flush(p, st, hs0, LB, E0, LN0, H0, LN0.hm, lo0, q0, count0, wide0, wg_off + before0);
    II2_STAMP(7)              // flush, tile 0
    if (work1 && !err && count1 != 0u) {
        if (!wide1) a2f_stage(st, hs1, LB, E1, LN1, H1, LN1.hm, lo1, q1);
        II2_STAMP(5)          // stage, tile 1
        a2f_flush(p, st, hs1, LB, E1, LN1, H1, LN1.hm, lo1, q1, count1, wide1, wg_off + total0 + before1);
        II2_STAMP(7)          // flush, tile 1
    }
    if (stamps && l == 0)
        for (int i = 0; i < 8; i++) atomicAdd(&p.debug[(uint64_t)(blockIdx.x % 2048u) * 8u + i], tacc[i]);
#undef II2_STAMP
}

// the ids of a tile's postings whose answer bit is set, into the wave's stage: 16-bit offsets from the tile's first doc, in output order
__device__ __forceinline__ void a2f_stage(uint16_t *st, const uint32_t *hs, const ListView &LB, const uint4 &EB, const A2Lane &LN, unsigned long long H,
                                          unsigned long long hm_any, uint32_t lo, uint32_t q0) {
    const unsigned long long He = LN.live ? H : 0ull;
    // 64 steps, the same for every lane: the running id advances by the gap byte (SDWA picks it), the answer word is
    // shifted left by adding it to itself — the bit that falls out is the step's write mask — and the lanes whose bit
    // was set store the id's 16-bit offset at their place and move on: 3 vector + 1 LDS + 2 scalar instructions a posting
    // (s_and_saveexec writes SCC: the clobber list says so — the compiler keeps branch conditions there across statements).
    // (The compiler's form of `if (bit) st[q++] = v` is 7 + 1 + 2.)
    uint32_t qa = (uint32_t)(uintptr_t)st + 2u * q0;        // (low 32 bits of an LDS pointer = its offset)
    uint32_t v = LN.base - lo;
    uint32_t h = __builtin_bitreverse32((uint32_t)He);
    unsigned long long sx;
    asm volatile("v_add_co_u32 %1, vcc, %1, %1\n\t"
                 "s_and_saveexec_b64 %3, vcc\n\t"
                 "ds_write_b16 %2, %0\n\t"
                 "v_add_u32 %2, 2, %2\n\t"
                 "s_mov_b64 exec, %3"
                 : "+v"(v), "+v"(h), "+v"(qa), "=&s"(sx) : : "vcc", "scc", "memory");
#define A2_STEP_TXT(SEL)                                                                                               \
    "v_add_u32_sdwa %0, %0, %4 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:" SEL "\n\t"           \
    "v_add_co_u32 %1, vcc, %1, %1\n\t"                                                                            \
    "s_and_saveexec_b64 %3, vcc\n\t"                                                                              \
    "ds_write_b16 %2, %0\n\t"                                                                                     \
    "v_add_u32 %2, 2, %2\n\t"                                                                                     \
    "s_mov_b64 exec, %3\n\t"
#define A2_STAGE_STEP(W, SEL) asm volatile(A2_STEP_TXT(SEL) : "+v"(v), "+v"(h), "+v"(qa), "=&s"(sx) : "v"(W) : "vcc", "scc", "memory");
#define A2_STAGE_3(W) asm volatile(A2_STEP_TXT("BYTE_0") A2_STEP_TXT("BYTE_1") A2_STEP_TXT("BYTE_2") : "+v"(v), "+v"(h), "+v"(qa), "=&s"(sx) : "v"(W) : "vcc", "scc", "memory");
#define A2_STAGE_WORD(W) asm volatile(A2_STEP_TXT("BYTE_0") A2_STEP_TXT("BYTE_1") A2_STEP_TXT("BYTE_2") A2_STEP_TXT("BYTE_3") : "+v"(v), "+v"(h), "+v"(qa), "=&s"(sx) : "v"(W) : "vcc", "scc", "memory");
    A2_STAGE_WORD(LN.ww[0]) A2_STAGE_WORD(LN.ww[1]) A2_STAGE_WORD(LN.ww[2]) A2_STAGE_WORD(LN.ww[3])
    A2_STAGE_WORD(LN.ww[4]) A2_STAGE_WORD(LN.ww[5]) A2_STAGE_WORD(LN.ww[6])
    A2_STAGE_3(LN.ww[7])                                                                                        // postings 1..31
    h = __builtin_bitreverse32((uint32_t)(He >> 32));
    A2_STAGE_STEP(LN.ww[7], "BYTE_3")
    A2_STAGE_WORD(LN.ww[8]) A2_STAGE_WORD(LN.ww[9]) A2_STAGE_WORD(LN.ww[10]) A2_STAGE_WORD(LN.ww[11])
    A2_STAGE_WORD(LN.ww[12]) A2_STAGE_WORD(LN.ww[13]) A2_STAGE_WORD(LN.ww[14])
    A2_STAGE_3(LN.ww[15])                                                                                       // postings 33..63
#undef A2_STAGE_WORD
#undef A2_STAGE_3
#undef A2_STAGE_STEP
#undef A2_STEP_TXT
    if (hm_any != 0ull) {                   // rows with multi-byte gaps: decoded again, every hit ranks itself among its row's answers
#pragma unroll 1
        for (uint32_t r = 0; r < A2_ROWS; r++) {
            if (((hm_any >> (4u * r)) & 0xFull) == 0ull) continue;
            const uint32_t fq = (uint32_t)__builtin_amdgcn_readlane((int)EB.x, (int)(4u * r)), q0r = (uint32_t)__builtin_amdgcn_readlane((int)EB.y, (int)(4u * r)),
                           q1r = (uint32_t)__builtin_amdgcn_readlane((int)EB.w, (int)(4u * r));
            const uint32_t qrow = (uint32_t)__builtin_amdgcn_readlane((int)q0, (int)(4u * r));
            const uint32_t *hr = hs + 8u * r;
            auto place = [&](uint32_t ix, uint32_t id) {
                if (ix >= 256u) return;
                const uint32_t wd = hr[ix >> 5];
                if (!((wd >> (ix & 31u)) & 1u)) return;
                uint32_t rk = (uint32_t)__popc(wd & ((1u << (ix & 31u)) - 1u));
                for (uint32_t j = 0; j < (ix >> 5); j++) rk += (uint32_t)__popc(hr[j]);
                st[qrow + rk] = (uint16_t)(id - lo);
            };
            decode_block_wave4(GlobalBytes{LB.payload}, q0r, q1r, fq,
                               [&](uint32_t ix, uint32_t id0, uint32_t id1, uint32_t id2, uint32_t id3, uint32_t mask) {
                                   if (mask & 1u) { place(ix, id0); ix++; }
                                   if (mask & 2u) { place(ix, id1); ix++; }
                                   if (mask & 4u) { place(ix, id2); ix++; }
                                   if (mask & 8u) { place(ix, id3); ix++; }
                               });
        }
    }
}

// a tile's staged ids out to their place (16 bytes per lane); a tile wider than 64 k docs has none staged: its ids go out one by one
__device__ __forceinline__ void a2f_flush(const DenseParams &p, const uint16_t *st, const uint32_t *hs, const ListView &LB, const uint4 &EB, const A2Lane &LN,
                                          unsigned long long H, unsigned long long hm_any, uint32_t lo, uint32_t q0, uint32_t count, bool wide,
                                          unsigned long long off) {
    const int l = lane_id();
    if (!wide) {
        const bool fits = off + count <= p.out_cap;
        for (uint32_t c = 4u * (uint32_t)l; c < count; c += 256u) {        // 16 bytes per lane (wave-private LDS: program order is enough)
            const uint2 pk = *reinterpret_cast<const uint2 *>(&st[c]);
            const uint4 ids = make_uint4(lo + (pk.x & 0xFFFFu), lo + (pk.x >> 16), lo + (pk.y & 0xFFFFu), lo + (pk.y >> 16));
            if (c + 4u <= count && fits) {
                uint32_t *dst = p.out + off + c;
                __builtin_memcpy(dst, &ids, 16);                // one 16-byte store, any 4-byte alignment
            } else {
                const uint32_t vv[4] = {ids.x, ids.y, ids.z, ids.w};
                for (uint32_t k = 0; k < 4u; k++)
                    if (c + k < count && off + c + k < p.out_cap) p.out[off + c + k] = vv[k];
            }
        }
    } else {
        const unsigned long long He = LN.live ? H : 0ull;
        uint32_t q = q0;
        uint32_t v = LN.base;
        if ((He & 1ull) && off + q < p.out_cap) p.out[off + q] = v;
        q += (uint32_t)(He & 1ull);
#pragma unroll
        for (uint32_t k = 0; k < 63u; k++) {
            v += (LN.ww[k >> 2] >> (8u * (k & 3u))) & 0xFFu;
            const uint32_t hit = (uint32_t)((He >> (k + 1u)) & 1ull);
            if (hit && off + q < p.out_cap) p.out[off + q] = v;
            q += hit;
        }
        if (hm_any != 0ull) {
#pragma unroll 1
            for (uint32_t r = 0; r < A2_ROWS; r++) {
                if (((hm_any >> (4u * r)) & 0xFull) == 0ull) continue;
                const uint32_t fq = (uint32_t)__builtin_amdgcn_readlane((int)EB.x, (int)(4u * r)), q0r = (uint32_t)__builtin_amdgcn_readlane((int)EB.y, (int)(4u * r)),
                               q1r = (uint32_t)__builtin_amdgcn_readlane((int)EB.w, (int)(4u * r));
                const uint32_t qrow = (uint32_t)__builtin_amdgcn_readlane((int)q0, (int)(4u * r));
                const uint32_t *hr = hs + 8u * r;
                auto place = [&](uint32_t ix, uint32_t id) {
                    if (ix >= 256u) return;
                    const uint32_t wd = hr[ix >> 5];
                    if (!((wd >> (ix & 31u)) & 1u)) return;
                    uint32_t rk = (uint32_t)__popc(wd & ((1u << (ix & 31u)) - 1u));
                    for (uint32_t j = 0; j < (ix >> 5); j++) rk += (uint32_t)__popc(hr[j]);
                    if (off + qrow + rk < p.out_cap) p.out[off + qrow + rk] = id;
                };
                decode_block_wave4(GlobalBytes{LB.payload}, q0r, q1r, fq,
                                   [&](uint32_t ix, uint32_t id0, uint32_t id1, uint32_t id2, uint32_t id3, uint32_t mask) {
                                       if (mask & 1u) { place(ix, id0); ix++; }
                                       if (mask & 2u) { place(ix, id1); ix++; }
                                       if (mask & 4u) { place(ix, id2); ix++; }
                                       if (mask & 8u) { place(ix, id3); ix++; }
                                   });
            }
        }
    }
}

// ---- the dense form of a list: its marking, done once ---------------------------------------------------------------
// A wave takes sixteen blocks of the list; its docs are [first doc of its first block, first doc of the next wave's first block)
// (the list's last doc for the last wave).  That range is cut into windows of A2_CAPW docs from its first doc & ~31 on (a sparse
// stretch makes many); per window the sixteen blocks are marked into the wave's LDS bitmap by a2_mark_rows - which takes any
// block and leaves out what lies outside the window - and the window's non-zero words are OR-ed into the global array.  The
// first and the last word of a wave's range are shared with its neighbours: every word goes out as a vector atomic (a one-off
// per list: exactness before speed).
__global__ __launch_bounds__(256) void k_dense_form_build(ListView LA, uint32_t origin, uint32_t n_words, uint32_t *bits) {
    __shared__ __align__(16) uint32_t lds[4][A2_NW];
    const int l = lane_id();
    const uint32_t wv = a2_uni(threadIdx.x >> 6);
    const uint32_t rl = (uint32_t)l & 3u, row = (uint32_t)l >> 2;
    const uint32_t a0 = (blockIdx.x * 4u + wv) * A2_ROWS;
    if (a0 >= LA.nblk) return;                               // wave-uniform; no barrier below
    uint32_t *lds_all = &lds[0][0];
    uint32_t *bm = lds[wv];
    const uint32_t nv = LA.nblk - a0 < A2_ROWS ? LA.nblk - a0 : A2_ROWS;
    const bool rv = row < nv;
    const uint4 E = a2_ent_load(LA, a0, row);
    const A2Bytes B = a2_fetch(LA.payload, rv, E.y, E.w, rl);
    const uint32_t lo = a2_uni(E.x);
    const uint32_t nf = (uint32_t)__builtin_amdgcn_readlane((int)E.z, (int)(4u * (nv - 1u)));
    const uint32_t hi = a0 + A2_ROWS < LA.nblk ? nf - 1u : a2_uni(*LA.last_doc);
    uint32_t wlo = lo & ~31u;
    for (;;) {
        const uint32_t wspan = hi - wlo < A2_CAPW ? hi - wlo : A2_CAPW - 1u;
        const uint32_t nw = (wspan >> 5) + 1u;
        const uint32_t ncl = nw + 2u * (A2_GU / 32u) + 2u;       // <= A2_NW - 2; cleared in 4-word steps
        for (uint32_t i = 4u * (uint32_t)l; i < ncl; i += 256u) *reinterpret_cast<uint4 *>(&bm[i]) = make_uint4(0, 0, 0, 0);
        a2_mark_rows(lds_all, bm, LA.payload, rv, E.x, E.y, E.w, B, wlo, wspan, rl, row);
        const uint32_t g0 = (wlo - origin) >> 5;                // (wlo >= origin: the list's first doc & ~31)
        for (uint32_t i = (uint32_t)l; i < nw; i += 64u) {
            const uint32_t wd = bm[A2_GU / 32u + i];
            if (wd != 0u && g0 + i < n_words) atomicOr(&bits[g0 + i], wd);
        }
        if (hi - wlo < A2_CAPW) break;
        wlo += A2_CAPW;
    }
}

hipError_t launch_dense_form_build(const ListView &L, uint32_t origin, uint32_t n_words, uint32_t *bits, hipStream_t s) {
    const uint32_t waves = (L.nblk + A2_ROWS - 1u) / A2_ROWS;
    hipLaunchKernelGGL(k_dense_form_build, dim3((waves + 3u) / 4u), dim3(256), 0, s, L, origin, n_words, bits);
    return hipGetLastError();
}

// workgroups of the one-tile dense-form instance that a CU holds at once, by the occupancy query (0: the query failed)
uint32_t and2_fused_wgs_per_cu() {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_and2_fused<true>, 256, 0) != hipSuccess) {
        (void)hipGetLastError();
        return 0u;
    }
    return n > 0 ? (uint32_t)n : 0u;
}

// one launch (the look-back records are set) or two kernels
Path intersect_and2_path(const DenseParams &p) { return p.lb.agg != nullptr ? P_AND_AND2_FUSED : P_AND_AND2_SPLIT; }

hipError_t launch_intersect_and2(const DenseParams &p, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (ev0) (void)hipEventRecord(ev0, s);
    const uint32_t grid = (p.n_waves + 3u) / 4u;
    if (intersect_and2_path(p) == P_AND_AND2_FUSED) {
        if (p.a_bits && p.b_bits) (void)launch_and2_words(p, s);     // both lists as bitmaps: intersect_words.hip
        else if (p.a_bits && p.and2_tiles == 2u) hipLaunchKernelGGL(k_and2_fused_x2, dim3((grid + 1u) / 2u), dim3(256), 0, s, p);
        else if (p.a_bits) hipLaunchKernelGGL(k_and2_fused<true>, dim3(grid), dim3(256), 0, s, p);
        else hipLaunchKernelGGL(k_and2_fused<false>, dim3(grid), dim3(256), 0, s, p);
        if (ev1) (void)hipEventRecord(ev1, s);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_and2_tiles, dim3(grid), dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_and2_expand, dim3(grid), dim3(256), 0, s, p);
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

}  // namespace ii2
