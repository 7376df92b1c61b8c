// intersect_ranges.hip — AND of ORs over list ranges (ii2_intersect_ranges): the filters of the group path.  The candidates
// (the union of the group with the fewest postings, setop.cpp) are an ascending id array; each further group is one pass
// that flags the candidates found in at least one of its lists, then scan.hip turns the flags into offsets in place and
// k_ir_compact writes the survivors in order.  An excluded group (ii2_andnot_ranges) is the same pass with the flag turned
// round (IrParams::drop): the candidates NOT found survive.  Two ways to flag:
//   probe (k_ir_probe): one wave per run of IR_PROBE_RUN consecutive candidates.  Per list of the group it finds the block of
//        its first open candidate with the guess-then-walk search (upper_bound_guess), then walks forward: the next 64 skip
//        entries in one load, a new search only past them.  Every block it lands on is decoded once into LDS and the open
//        candidates inside the block's doc range are looked up there.  A list whose span misses the run costs nothing.
//   mark (k_um_mark of union_many.hip + k_ir_test + k_ir_clear): the group's blocks that overlap the window are marked into
//        the per-context doc bitmap, every candidate tests its bit, then the words and summary words set are zeroed again.
// No kernel waits for another workgroup.
#include <hip/hip_runtime.h>

#include "dv1_device.h"
#include "internal.h"

namespace ii2 {

__global__ __launch_bounds__(256) void k_ir_probe(IrParams p) {
    __shared__ uint32_t stage[4][II2_DV1_BLOCK];
    constexpr uint32_t CH = IR_PROBE_RUN / 64u;                         // candidates per lane
    const uint32_t l = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t c0 = ((uint64_t)blockIdx.x * 4u + wv) * IR_PROBE_RUN;
    if (c0 >= p.n_cand) return;                                           // (wave-uniform; no workgroup barrier below)
    uint32_t *s = stage[wv];
    uint32_t x[CH];
    bool valid[CH], found[CH];
#pragma unroll
    for (uint32_t k = 0; k < CH; k++) {
        const uint64_t i = c0 + k * 64u + l;
        valid[k] = i < p.n_cand;
        x[k] = valid[k] ? p.cand[i] : 0u;
        found[k] = false;
    }
    const uint64_t c_last = (c0 + IR_PROBE_RUN < p.n_cand ? c0 + IR_PROBE_RUN : p.n_cand) - 1u;
    const uint32_t run_lo = wave_bcast(x[0], 0), run_hi = p.cand[c_last];
    for (uint32_t li = 0; li < p.n_lists; li++) {
        const IrList L = p.lists[li];
        uint32_t lo = L.lo, hi = L.hi;
        if (lo > hi) {                                                    // span not mirrored on the host: from the list itself
            lo = L.skip[0].first_doc;
            hi = *L.last_doc;
        }
        if (hi < run_lo || lo > run_hi) continue;
        auto get = [&](uint32_t j) { return L.skip[j].first_doc; };
        uint32_t b = 0xFFFFFFFFu;                                         // block decoded into s (none yet)
        uint64_t b_end = 0;                                               // one past its last doc
        uint32_t nb = 0;                                                  // its postings
#pragma unroll
        for (uint32_t k = 0; k < CH; k++) {
            bool open = valid[k] && !found[k] && x[k] >= lo && x[k] <= hi;
            for (unsigned long long m = __ballot(open); m; m = __ballot(open)) {
                const uint32_t xm = wave_bcast(x[k], __ffsll((long long)m) - 1);   // the smallest open candidate
                if (b == 0xFFFFFFFFu || (uint64_t)xm >= b_end) {
                    uint32_t nbk;
                    if (b == 0xFFFFFFFFu) {
                        nbk = upper_bound_guess(get, 0u, L.nblk, xm, lo, hi) - 1u;      // xm >= lo: at least block 0
                    } else {
                        // walk: the next 64 blocks' first docs in one load; their prefix <= xm holds xm's block (lanes past the
                        // list's last block never count, not even for xm = 2^32 - 1: ahead == 64 only when 64 real blocks follow b)
                        const uint32_t j = b + 1u + l;
                        const bool in_list = j < L.nblk;
                        const uint32_t fd = in_list ? L.skip[j].first_doc : 0u;
                        const uint32_t ahead = (uint32_t)__popcll(__ballot(in_list && fd <= xm));
                        if (ahead < 64u) nbk = b + ahead;
                        else nbk = upper_bound_guess(get, b + 65u, L.nblk, xm, wave_bcast(fd, 63), hi) - 1u;
                    }
                    b = nbk;
                    const ii2_skip e0 = L.skip[b], e1 = L.skip[b + 1u];
                    b_end = b + 1u < L.nblk ? (uint64_t)e1.first_doc : (uint64_t)hi + 1u;
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");         // the last block's reads before this block's writes
                    nb = decode_block_wave4(GlobalBytes{L.payload}, e0.byte_off, e1.byte_off, e0.first_doc,
                                            [&](uint32_t ix, uint32_t id0, uint32_t id1, uint32_t id2, uint32_t id3, uint32_t mask) {
                                                if ((mask & 1u) && ix < II2_DV1_BLOCK) s[ix] = id0;
                                                ix += mask & 1u;
                                                if ((mask & 2u) && ix < II2_DV1_BLOCK) s[ix] = id1;
                                                ix += (mask >> 1) & 1u;
                                                if ((mask & 4u) && ix < II2_DV1_BLOCK) s[ix] = id2;
                                                ix += (mask >> 2) & 1u;
                                                if ((mask & 8u) && ix < II2_DV1_BLOCK) s[ix] = id3;
                                            });
                    nb = nb < II2_DV1_BLOCK ? nb : II2_DV1_BLOCK;
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");         // the wave's LDS writes before its reads of other lanes' ids
                }
                if (open && (uint64_t)x[k] < b_end) {                     // inside the decoded block: look it up
                    uint32_t a = 0, e = nb;
                    while (a < e) { const uint32_t mid = (a + e) >> 1; if (s[mid] < x[k]) a = mid + 1u; else e = mid; }
                    found[k] = a < nb && s[a] == x[k];
                    open = false;
                }
            }
        }
        bool all = true;
#pragma unroll
        for (uint32_t k = 0; k < CH; k++) all = all && (!valid[k] || found[k]);
        if (__ballot(!all) == 0ull) break;
    }
#pragma unroll
    for (uint32_t k = 0; k < CH; k++)
        if (valid[k]) p.flag[c0 + k * 64u + l] = (found[k] ? 1u : 0u) ^ p.drop;      // (an exclusion keeps what was NOT found)
}

// mark mode: every candidate inside the window whose bit the group's blocks set is flagged (flags start at zero); an exclusion
// (p.drop) starts them at one - a candidate outside every window survives - and a set bit clears the flag
__global__ __launch_bounds__(256) void k_ir_test(IrParams p) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= p.n_cand) return;
    const uint32_t rel = p.cand[i] - p.win_lo;
    if (p.cand[i] < p.win_lo || rel >= p.win_docs) return;
    if ((p.bitmap[rel >> 5] >> (rel & 31u)) & 1u) p.flag[i] = 1u ^ p.drop;
}

// mark mode: the scratch back to zero - one wave per summary word, as k_um_compact clears it
__global__ __launch_bounds__(256) void k_ir_clear(IrParams p) {
    const uint32_t l = threadIdx.x & 63u;
    const uint32_t n_waves = gridDim.x * 4u;
    for (uint32_t sw = blockIdx.x * 4u + (threadIdx.x >> 6); sw < p.n_sum; sw += n_waves) {
        uint32_t bits = p.summary[sw];
        if (!bits) continue;
        while (bits) {
            const uint32_t chunk = (uint32_t)__builtin_ctz(bits);
            bits &= bits - 1u;
            const uint32_t wi = (sw * 32u + chunk) * 64u + l;
            if (p.bitmap[wi]) p.bitmap[wi] = 0u;
        }
        if (l == 0) p.summary[sw] = 0u;
    }
}

// the survivors in order: flag[] holds the exclusive scan of the flags (flag[n_cand] = their total); all or nothing
__global__ __launch_bounds__(256) void k_ir_compact(IrParams p) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t total = p.flag[p.n_cand];
    if (i == 0) *p.d_count = total;
    if (i >= p.n_cand || total > p.out_cap) return;
    const uint32_t at = p.flag[i];
    if (p.flag[i + 1u] != at) p.out[at] = p.cand[i];
}

hipError_t launch_ir_probe(const IrParams &p, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    const uint64_t waves = (p.n_cand + IR_PROBE_RUN - 1u) / IR_PROBE_RUN;
    if (ev0) (void)hipEventRecord(ev0, s);
    hipLaunchKernelGGL(k_ir_probe, dim3((unsigned)((waves + 3u) / 4u)), dim3(256), 0, s, p);
    if (ev1) (void)hipEventRecord(ev1, s);
    return hipGetLastError();
}

hipError_t launch_ir_test(const IrParams &p, hipStream_t s) {
    hipLaunchKernelGGL(k_ir_test, dim3((unsigned)((p.n_cand + 255u) / 256u)), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_ir_clear(const IrParams &p, uint32_t grid, hipStream_t s) {
    hipLaunchKernelGGL(k_ir_clear, dim3(grid), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_ir_compact(const IrParams &p, hipStream_t s) {
    hipLaunchKernelGGL(k_ir_compact, dim3((unsigned)((p.n_cand + 255u) / 256u)), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace ii2
